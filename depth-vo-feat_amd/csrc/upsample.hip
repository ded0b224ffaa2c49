// Integer-factor bilinear upsampling (x2, x4, x8) of a coarse map to the input resolution, optionally fused with the
// disparity -> depth reciprocal: the full-resolution multi-scale mode of the photometric losses (build-side extension, the
// reference has no such mode; definition: tests/fullres_ref.py).
//   forward   out = up(in)                      or   out = 1 / (up(in) + eps)      one thread per fine pixel
//   backward  gin = up^T(gout)                  or   gin = up^T(-gout * out^2)     gather form, separable, no atomics
// The backward is the exact transpose of the forward.  A block owns RC x TC coarse pixels of one plane, i.e. a 32 x 128 core
// of fine pixels plus a halo of F/2 on every side (a coarse pixel collects from 2F x 2F fine ones).  It
//   1. reads its (32 + F) x (128 + F) fine tile once, coalesced along X, into LDS (out-of-image = 0, the reciprocal's
//      -out^2 applied on the way in),
//   2. row pass: every (fine row, coarse column) sums its 2F horizontal taps in ascending X          -> LDS,
//   3. column pass: every coarse pixel sums its 2F vertical taps of those row sums in ascending Y    -> gin, written once.
// Every sum has a fixed order, so the result is bit-reproducible.  The halo makes neighbouring blocks read (1 + F/32) x
// (1 + F/128) of the core from L2; HBM sees each fine pixel once.
// LDS: tile column c of a row lives at c + c / F, so the row pass (lane = coarse column, window start F * lane) walks the
// banks with the odd stride F + 1 instead of F: conflict-free ds_read_b32.  Largest footprint (F = 2): 34 x 196 + 34 x 64
// floats = 35 KiB, four blocks per CU.
#include "bilinear_src.h"
#include "dvf_common.h"

namespace {

constexpr int CORE_H = 32, CORE_W = 128, THREADS = 256;

template <int F, bool RECIP>
__global__ void upsample_int_fwd_kernel(const float *__restrict__ in, float *__restrict__ out, int H, int W, uint32_t total,
                                        float eps) {
    const uint32_t OW = (uint32_t)(F * W), OH = (uint32_t)(F * H);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const uint32_t row = i / OW, plane = row / OH;
        const int X = (int)(i - row * OW), Y = (int)(row - plane * OH);
        int y0, y1, x0, x1;
        float ly, lx;
        up_src(Y, 1.f / F, H, y0, y1, ly);
        up_src(X, 1.f / F, W, x0, x1, lx);
        const float *p = in + (int64_t)plane * H * W;
        const float top = (1.f - lx) * p[y0 * W + x0] + lx * p[y0 * W + x1];
        const float bot = (1.f - lx) * p[y1 * W + x0] + lx * p[y1 * W + x1];
        const float v = (1.f - ly) * top + ly * bot;
        out[i] = RECIP ? 1.f / (v + eps) : v;
    }
}

// weight with which fine index `fine` (of `fine_size` = F * in_size) feeds coarse index `coarse`; 0 outside the image
template <int F>
__device__ __forceinline__ float tap_weight(int fine, int coarse, int in_size) {
    if (fine < 0 || fine >= F * in_size) return 0.f;
    int a0, a1;
    float l;
    up_src(fine, 1.f / F, in_size, a0, a1, l);
    return (a0 == coarse ? 1.f - l : 0.f) + (a1 == coarse ? l : 0.f);
}

template <int F, bool RECIP>
__global__ __launch_bounds__(THREADS) void upsample_int_bwd_kernel(const float *__restrict__ gout,
                                                                   const float *__restrict__ out, float *__restrict__ gin,
                                                                   int H, int W, int tiles_x, int tiles_y) {
    constexpr int LOGF = F == 2 ? 1 : (F == 4 ? 2 : 3);
    constexpr int RC = CORE_H / F, TC = CORE_W / F;            // coarse rows / columns of a block
    constexpr int FH = CORE_H + F, FW = CORE_W + F;            // fine tile with its halo
    constexpr int S1 = FW + FW / F + 1;                        // padded row stride of the fine tile
    __shared__ float tile[FH * S1];
    __shared__ float rowsum[FH * TC];
    const int OH = F * H, OW = F * W;
    const int bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, plane = blockIdx.x / (tiles_x * tiles_y);
    const int cx0 = bx * TC, cy0 = by * RC;                    // first coarse column / row of this block
    const int X0 = F * cx0 - F / 2, Y0 = F * cy0 - F / 2;      // fine coordinates of tile element (0, 0)
    const int tid = threadIdx.x;
    const int64_t fine_base = (int64_t)plane * OH * OW;

    for (int i = tid; i < FH * FW; i += THREADS) {
        const int r = i / FW, c = i - r * FW;
        const int Y = Y0 + r, X = X0 + c;
        float v = 0.f;
        if (Y >= 0 && Y < OH && X >= 0 && X < OW) {
            const int64_t off = fine_base + (int64_t)Y * OW + X;
            v = gout[off];
            if (RECIP) {
                const float o = out[off];
                v = -v * o * o;
            }
        }
        tile[r * S1 + c + (c >> LOGF)] = v;
    }
    __syncthreads();

    {   // row pass: this thread's coarse column, every (THREADS / TC)-th fine row
        const int xl = tid % TC, x = cx0 + xl;
        float wx[2 * F];
#pragma unroll
        for (int k = 0; k < 2 * F; ++k) wx[k] = x < W ? tap_weight<F>(X0 + F * xl + k, x, W) : 0.f;
        for (int r = tid / TC; r < FH; r += THREADS / TC) {
            const float *t = tile + r * S1 + (F + 1) * xl;     // column F * xl + k sits at (F + 1) * xl + k + (k >= F)
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 2 * F; ++k) s += wx[k] * t[k + (k >= F ? 1 : 0)];
            rowsum[r * TC + xl] = s;
        }
    }
    __syncthreads();

    for (int o = tid; o < RC * TC; o += THREADS) {   // column pass
        const int yl = o / TC, xl = o - yl * TC;
        const int y = cy0 + yl, x = cx0 + xl;
        if (y >= H || x >= W) continue;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 2 * F; ++k) s += tap_weight<F>(Y0 + F * yl + k, y, H) * rowsum[(F * yl + k) * TC + xl];
        gin[(int64_t)plane * H * W + (int64_t)y * W + x] = s;
    }
}

inline int nblocks(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

// host-side argument checks shared by both entries: 0 or a DVF_ERR_* code; touches no GPU
inline int check_sizes(int planes, int H, int W, int factor) {
    if (planes <= 0 || H <= 0 || W <= 0) return DVF_ERR_INVALID_ARG;
    if (factor != 2 && factor != 4 && factor != 8) return DVF_ERR_UNSUPPORTED;
    // the kernels index fine pixels in 32 bits
    if ((int64_t)planes * H * W * factor * factor >= ((int64_t)1 << 31)) return DVF_ERR_INVALID_ARG;
    return DVF_OK;
}

template <int F>
int launch_fwd(const float *in, float *out, int planes, int H, int W, int recip, float eps, hipStream_t st) {
    const uint32_t total = (uint32_t)planes * H * W * F * F;
    if (recip)
        upsample_int_fwd_kernel<F, true><<<nblocks(total), 256, 0, st>>>(in, out, H, W, total, eps);
    else
        upsample_int_fwd_kernel<F, false><<<nblocks(total), 256, 0, st>>>(in, out, H, W, total, eps);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

template <int F>
int launch_bwd(const float *gout, const float *out, float *gin, int planes, int H, int W, int recip, hipStream_t st) {
    const int tiles_x = (W + CORE_W / F - 1) / (CORE_W / F), tiles_y = (H + CORE_H / F - 1) / (CORE_H / F);
    const int blocks = tiles_x * tiles_y * planes;             // < 2^31 / (32 * 128): check_sizes bounds the fine pixels
    if (recip)
        upsample_int_bwd_kernel<F, true><<<blocks, THREADS, 0, st>>>(gout, out, gin, H, W, tiles_x, tiles_y);
    else
        upsample_int_bwd_kernel<F, false><<<blocks, THREADS, 0, st>>>(gout, out, gin, H, W, tiles_x, tiles_y);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

}  // namespace

extern "C" {

int dvf_upsample_int_fwd(const float *in, float *out, int planes, int H, int W, int factor, int recip, float eps,
                         void *stream) {
    if (!in || !out) return DVF_ERR_INVALID_ARG;
    if (const int rc = check_sizes(planes, H, W, factor)) return rc;
    hipStream_t st = dvf_stream(stream);
    return factor == 2 ? launch_fwd<2>(in, out, planes, H, W, recip, eps, st)
         : factor == 4 ? launch_fwd<4>(in, out, planes, H, W, recip, eps, st)
                       : launch_fwd<8>(in, out, planes, H, W, recip, eps, st);
}

int dvf_upsample_int_bwd(const float *gout, const float *out, float *gin, int planes, int H, int W, int factor, int recip,
                         void *stream) {
    if (!gout || !gin || (recip && !out)) return DVF_ERR_INVALID_ARG;
    if (const int rc = check_sizes(planes, H, W, factor)) return rc;
    hipStream_t st = dvf_stream(stream);
    return factor == 2 ? launch_bwd<2>(gout, out, gin, planes, H, W, recip, st)
         : factor == 4 ? launch_bwd<4>(gout, out, gin, planes, H, W, recip, st)
                       : launch_bwd<8>(gout, out, gin, planes, H, W, recip, st);
}

}  // extern "C"
