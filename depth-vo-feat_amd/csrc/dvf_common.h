// Shared helpers for the libdvf_hip.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>

#include "../../include/dvf_hip.h"

#define DVF_LAUNCH_CHECK()                                   \
    do {                                                     \
        if (hipGetLastError() != hipSuccess) return DVF_ERR_LAUNCH; \
    } while (0)

static inline hipStream_t dvf_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Tuning knobs and ablation switches exist only in a -DDVF_TUNING build (`make TUNING=1`, used by tools/): the product
// library reads no environment variable on a launch path and carries no code that can switch parts of a kernel off.
#ifdef DVF_TUNING
static inline const char *dvf_tune(const char *name) { return getenv(name); }
#define DVF_DBG(a, bit) ((a).dbg & (bit))
#else
static inline const char *dvf_tune(const char *) { return nullptr; }
#define DVF_DBG(a, bit) (0)
#endif

// Plan log: every convolution entry point notes which kernel family and tiling it launched (thread-local, reset at the
// entry); dvf_conv2d_last_plans() reads it back.  Tests use it to prove that the plans exercised by the parity cases
// are the plans the benchmark step runs.  The record layout is the table above dvf_conv2d_last_plans in include/dvf_hip.h;
// the dvf_note_* functions below are the only places that give a field its position.
struct DvfPlanLog { int n; int rec[DVF_PLAN_MAX][DVF_PLAN_INTS]; };
DvfPlanLog &dvf_plan_log();
static inline void dvf_plan_reset() { dvf_plan_log().n = 0; }
static inline void dvf_plan_note(int kernel, int a = 0, int b = 0, int c = 0, int d = 0, int e = 0, int f = 0, int g = 0,
                                 int h = 0, int i = 0, int j = 0, int k = 0) {      // private to the note functions
    DvfPlanLog &l = dvf_plan_log();
    if (l.n >= DVF_PLAN_MAX) return;
    const int v[DVF_PLAN_INTS] = {kernel, a, b, c, d, e, f, g, h, i, j, k};
    for (int x = 0; x < DVF_PLAN_INTS; ++x) l.rec[l.n][x] = v[x];
    ++l.n;
}

constexpr int dvf_pipe_plan_flags(int out_mode, int ncls, int x4, int blocked, int lr, int npi) {
    return out_mode | (ncls << DVF_PLAN_NCLS_SHIFT) | (x4 << DVF_PLAN_X4_SHIFT) | (blocked << DVF_PLAN_BLOCKED_SHIFT) |
           (lr << DVF_PLAN_LR_SHIFT) | (npi << DVF_PLAN_NPI_SHIFT);
}
constexpr int dvf_wgrad_plan_tile(int MT, int TILE) { return MT | (TILE << DVF_PLAN_WG_TILE_SHIFT); }
constexpr int dvf_wgrad_plan_lanes(int x4, int ordered) { return (x4 << DVF_PLAN_WG_X4_SHIFT) | (ordered << DVF_PLAN_WG_ORDERED_SHIFT); }
static_assert(dvf_pipe_plan_flags(2, 4, 1, 1, 1, 12) == (2 | 4 << 4 | 1 << 8 | 1 << 9 | 1 << 10 | 12 << 11), "conv_pipe flags moved");
static_assert(dvf_pipe_plan_flags(1, 4, 0, 0, 0, 0) == (1 | 4 << 4), "conv_gather flags moved");
static_assert(dvf_wgrad_plan_tile(2, 32) == (2 | 32 << 8), "wgrad_pipe tile word moved");
static_assert(dvf_wgrad_plan_lanes(1, 1) == (1 | 2) && dvf_wgrad_plan_lanes(0, 1) == 2, "wgrad_pipe lanes word moved");

static inline void dvf_note_pipe(int MT, int NT, int WM, int CK, int TBU, int KS, int BN, int NST, int threads, int lds,
                                 int out_mode, int ncls, int x4, bool blocked, int lr, int npi) {
    dvf_plan_note(DVF_K_PIPE, MT, NT, WM, CK, TBU, KS, BN, NST, threads, lds, dvf_pipe_plan_flags(out_mode, ncls, x4, blocked, lr, npi));
}
static inline void dvf_note_gather(int MT, int NT, int CK, int KS, int lds, int out_mode, int ncls) {
    dvf_plan_note(DVF_K_GATHER, MT, NT, 1, CK, 0, KS, 1, 1, 256, lds, dvf_pipe_plan_flags(out_mode, ncls, 0, 0, 0, 0));
}
static inline void dvf_note_wgrad_pipe(int MT, int TILE, int NTW, int x4, bool ordered, int CK, int stride, int pieces, int blocks,
                                       int lds, int taps, int row_stride, int nseg) {
    dvf_plan_note(DVF_K_WGRAD_PIPE, dvf_wgrad_plan_tile(MT, TILE), NTW, dvf_wgrad_plan_lanes(x4, ordered), CK, stride, pieces, blocks,
                  lds, taps, row_stride, nseg);
}
static inline void dvf_note_wgrad_reg(int MT, int NTW, bool prefetch, int CK, int BH, int PSPLIT, int vec_p, int stride, int lds,
                                      int taps) {
    dvf_plan_note(DVF_K_WGRAD, MT, NTW, prefetch, CK, BH, PSPLIT, vec_p, stride, 256, lds, taps);
}
// the direct kernels of conv_head.hip: head_fwd (C_out, nseg), head_dgrad (C_out), head_wgrad (C_out, ordered),
// head_seg_dgrad (segc), dconvt_fwd (C_out, KH)
static inline void dvf_note_head(int kernel, int a, int b = 0) { dvf_plan_note(kernel, a, b); }

// Sum over the 64 lanes of a wave; every lane ends with the total.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Fixed-order sum over a 256-thread block (four waves): wave_sum, one float per wave into red[4], then (r0 + r1) + (r2 + r3);
// every thread returns the total.  `wave` is the caller's wave index (threadIdx.x >> 6 in a 1-D block, threadIdx.y in a
// 64x4 one).  A caller that uses the same `red` again puts a __syncthreads() between the two calls.
__device__ __forceinline__ float block_sum(float v, int wave, float *red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// Sum of partials[i * stride + offset], i < n, by a 1-D block of 256 threads: thread t adds i = t, t + 256, ... in that order,
// then block_sum.
__device__ __forceinline__ float block_sum_strided(const float *partials, int64_t n, int stride, int offset, float *red) {
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += partials[i * stride + offset];
    return block_sum(s, threadIdx.x >> 6, red);
}

// Row-major index of this block in its grid: the slot of its record in a per-block partials array.
__device__ __forceinline__ int64_t linear_block() {
    return ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
}

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// loss_out[0] (+)= scale * sum(partials[0 .. nblk)): the one-block second stage of the two-stage loss sums (elementwise.hip).
int dvf_sum_partials(const float *partials, int64_t nblk, float scale, float *loss_out, int accumulate, hipStream_t st);

// Image-shaped loss inputs: a grid with the B images in z, planes of at least min_side x min_side, 32-bit offsets within an
// image.  (fill_photo_args of photo_loss.hip spells the same test out: it reports the last clause as DVF_ERR_UNSUPPORTED.)
static inline bool image_shape_ok(int B, int C, int H, int W, int min_side) {
    return B > 0 && C > 0 && H >= min_side && W >= min_side && B <= 65535 && (int64_t)C * H * W < ((int64_t)1 << 31);
}
