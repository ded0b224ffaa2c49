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
// are the plans the benchmark step runs.
enum { DVF_K_PIPE = 1, DVF_K_GATHER = 2, DVF_K_HEAD_FWD = 3, DVF_K_HEAD_DGRAD = 4, DVF_K_HEAD_WGRAD = 5, DVF_K_WGRAD = 6,
       DVF_K_HEAD_SEG_DGRAD = 7, DVF_K_WGRAD_PIPE = 8, DVF_K_DCONVT_FWD = 9 };
constexpr int DVF_PLAN_INTS = 12, DVF_PLAN_MAX = 8;
struct DvfPlanLog { int n; int rec[DVF_PLAN_MAX][DVF_PLAN_INTS]; };
DvfPlanLog &dvf_plan_log();
static inline void dvf_plan_reset() { dvf_plan_log().n = 0; }
static inline void dvf_plan_note(int kernel, int a = 0, int b = 0, int c = 0, int d = 0, int e = 0, int f = 0, int g = 0,
                                 int h = 0, int i = 0, int j = 0, int k = 0) {
    DvfPlanLog &l = dvf_plan_log();
    if (l.n >= DVF_PLAN_MAX) return;
    const int v[DVF_PLAN_INTS] = {kernel, a, b, c, d, e, f, g, h, i, j, k};
    for (int x = 0; x < DVF_PLAN_INTS; ++x) l.rec[l.n][x] = v[x];
    ++l.n;
}

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
