// Opt-in appearance term, second part: per-pixel MINIMUM over the reference views of alpha * DSSIM + (1 - alpha) * L1, with
// an optional identity-reprojection auto-mask (monodepth2 form; like ssim_loss.hip there is no reference call site and
// parity is UNPINNED; tests/minreproj_ref.py is the definition and tests/ check this kernel pair against it in fp64).
// x = fl(in_scale * tgt); candidates y_k = fl(in_scale * cand[k]), k < K: the V warped references, then -- auto-mask -- the V
// unwarped ones (K = V or 2V).  Per pixel p:
//   e_k(p)  = (1/C) sum_c [alpha * dssim_c(x, y_k)(p) + (1 - alpha) * |x_c(p) - y_k,c(p)|]      (dssim: ssim_window.h)
//   usable  : a warped candidate unless it is exactly zero in all channels at p; an identity candidate always
//   k*(p)   = the LOWEST index among the usable candidates that attain min_k e_k(p)  (255 = none usable)
//   loss    = sum_p e_k*(p)(p) / (B H W)                 (pixels with no usable candidate add 0, stay in the denominator)
// The selection is piecewise constant: the backward routes each window's gradient to the candidate that won it.
//
// Forward: one launch; a block owns a 64x16 pixel tile of one image and walks candidates x channels with a running minimum
// and argmin per pixel (four vertically adjacent pixels per thread).  The target planes are staged once per block when
// all C fit in the LDS budget (C <= 3), else once per candidate.  Per block one loss partial and K+1 integer selection
// counts, reduced in a fixed order by a second one-block launch: loss and counts are bit-reproducible, no atomics.
// Backward: ONE launch that walks channels (outer) and candidates (inner), not one launch per view: g_tgt sums the
// selected candidate of every window over ALL candidates, so only a kernel that sees them all can write each g_tgt element
// exactly once; the target plane is then staged once per channel instead of once per candidate, and g_tgt needs four
// accumulators per thread for any C.  It is the gather of ssim_bwd_kernel with the ring weight valid * mask * g / N
// replaced by [select(q) = k] * g / N; a ring window is evaluated only for the candidate that won it.
#include "ssim_window.h"

namespace {

constexpr int MAX_V = 4, MAX_K = 2 * MAX_V;
constexpr int XP = 3;                         // target planes kept in LDS by the forward (3 x 5.1 KB)
constexpr int PLANE1 = (TH + 2) * SW;         // one halo-1 plane
constexpr int NONE = 255;

struct MinReprojPtrs {
    const float *cand[MAX_K];
    float *g[MAX_V];
};

__global__ __launch_bounds__(NT) void minreproj_fwd_kernel(const float *tgt, MinReprojPtrs a, int V, int K, uint8_t *select,
                                                           float *partials, int *cnt_partials, int C, int H, int W, float in_scale,
                                                           float alpha, float c1, float c2, int vec) {
    __shared__ __attribute__((aligned(16))) float sx[XP * PLANE1];
    __shared__ __attribute__((aligned(16))) float sy[PLANE1];
    __shared__ float red[NT / 64];
    __shared__ int redc[NT / 64][MAX_K + 1];
    const int n = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int lx = threadIdx.x & 63, ly0 = (threadIdx.x >> 6) * 4, gx = x0 + lx;
    const int64_t plane = (int64_t)H * W;
    const float *X = tgt + (int64_t)n * C * plane;
    const bool keep_x = C <= XP;
    if (keep_x)
        for (int c = 0; c < C; ++c) stage_plane<1>(sx + c * PLANE1, X + c * plane, H, W, y0, x0, in_scale, vec);
    float best[4] = {0.f, 0.f, 0.f, 0.f};
    int sel[4] = {NONE, NONE, NONE, NONE};
    for (int k = 0; k < K; ++k) {
        const float *Y = a.cand[k] + (int64_t)n * C * plane;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        const bool identity = k >= V;
        bool usable[4] = {identity, identity, identity, identity};
        for (int c = 0; c < C; ++c) {
            __syncthreads();
            if (!keep_x) stage_plane<1>(sx, X + c * plane, H, W, y0, x0, in_scale, vec);
            stage_plane<1>(sy, Y + c * plane, H, W, y0, x0, in_scale, vec);
            __syncthreads();
            const float *px = keep_x ? sx + c * PLANE1 : sx;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (gx >= W || y0 + ly0 + r >= H) continue;
                const int o = (ly0 + r) * SW + lx + 3;
                const SsimWin w = ssim_window(px, sy, o, c1, c2);
                const float xc = px[o + SW + 1], yc = sy[o + SW + 1];
                acc[r] += alpha * w.dssim + (1.f - alpha) * fabsf(xc - yc);
                usable[r] |= (yc != 0.f);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (usable[r] && (sel[r] == NONE || acc[r] < best[r])) {     // strict <: a tie stays with the lower index
                best[r] = acc[r];
                sel[r] = k;
            }
    }
    float s = 0.f;
    bool inside[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int gy = y0 + ly0 + r;
        inside[r] = gx < W && gy < H;
        if (!inside[r]) continue;
        select[(int64_t)n * plane + (int64_t)gy * W + gx] = (uint8_t)sel[r];
        if (sel[r] != NONE) s += best[r];
    }
    s = wave_sum(s);                                                    // block_sum written out: the counts share its barrier
    if (lx == 0) red[threadIdx.x >> 6] = s;
    for (int cat = 0; cat <= K; ++cat) {                                // cat == K counts "none"
        const int want = cat < K ? cat : NONE;
        int cnt = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) cnt += __popcll(__ballot(inside[r] && sel[r] == want));
        if (lx == 0) redc[threadIdx.x >> 6][cat] = cnt;
    }
    __syncthreads();
    const int64_t nblk = (int64_t)gridDim.x * gridDim.y * gridDim.z, blk = linear_block();
    if (threadIdx.x == 0) partials[blk] = (red[0] + red[1]) + (red[2] + red[3]);
    if (threadIdx.x <= K)
        cnt_partials[threadIdx.x * nblk + blk] = redc[0][threadIdx.x] + redc[1][threadIdx.x] + redc[2][threadIdx.x] + redc[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void minreproj_reduce_kernel(const float *partials, const int *cnt_partials, int64_t nblk, int K,
                                                               float scale, float *loss_out, int *counts, int accumulate) {
    __shared__ float red[4];
    __shared__ int redc[4];
    const float t = block_sum_strided(partials, nblk, 1, 0, red) * scale;
    if (threadIdx.x == 0) loss_out[0] = accumulate ? loss_out[0] + t : t;
    for (int cat = 0; cat <= K; ++cat) {
        int c = 0;
        for (int64_t i = threadIdx.x; i < nblk; i += 256) c += cnt_partials[cat * nblk + i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) redc[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) counts[cat] = redc[0] + redc[1] + redc[2] + redc[3];
    }
}

__global__ __launch_bounds__(NT) void minreproj_bwd_kernel(const float *tgt, MinReprojPtrs a, int V, int K, const uint8_t *select,
                                                           const float *grad_loss, float *g_tgt, int C, int H, int W, float in_scale,
                                                           float alpha, float c1, float c2, float inv_n, int vec) {
    __shared__ __attribute__((aligned(16))) float sx[(TH + 4) * SW];
    __shared__ __attribute__((aligned(16))) float sy[(TH + 4) * SW];
    __shared__ __attribute__((aligned(16))) float4 coef[RH * RW];   // (Px, Py, Q, R) of each ring window, weighted
    __shared__ int ssel[RH * RW];                                   // selection of each ring pixel (NONE outside the image)
    const int n = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int lx = threadIdx.x & 63, ly0 = (threadIdx.x >> 6) * 4, gx = x0 + lx;
    const int64_t plane = (int64_t)H * W;
    const float *X = tgt + (int64_t)n * C * plane;
    const float gl = grad_loss[0] * inv_n;

    for (int i = threadIdx.x; i < RH * RW; i += NT) {
        const int qy = y0 - 1 + i / RW, qx = x0 - 1 + i % RW;
        ssel[i] = (qy >= 0 && qy < H && qx >= 0 && qx < W) ? (int)select[(int64_t)n * plane + (int64_t)qy * W + qx] : NONE;
    }
    for (int c = 0; c < C; ++c) {
        float gt[4] = {0.f, 0.f, 0.f, 0.f};
        bool x_staged = false;
        for (int k = 0; k < K; ++k) {
            float *G = k < V ? a.g[k] : nullptr;
            if (!G && !g_tgt) continue;                             // (block-uniform) nothing to write for this candidate
            const float *Y = a.cand[k] + (int64_t)n * C * plane;
            __syncthreads();
            if (!x_staged) stage_plane<2>(sx, X + c * plane, H, W, y0, x0, in_scale, vec);
            x_staged = true;
            stage_plane<2>(sy, Y + c * plane, H, W, y0, x0, in_scale, vec);
            __syncthreads();
            for (int i = threadIdx.x; i < RH * RW; i += NT) {
                float4 kf = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ssel[i] == k) {                                 // in the image, and this candidate won the window
                    kf = ring_coef(ssim_window(sx, sy, (i / RW) * SW + i % RW + 2, c1, c2), alpha, gl);
                }
                coef[i] = kf;
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ly = ly0 + r, gy = y0 + ly;
                if (gx >= W || gy >= H) continue;
                // ring_gather (ssim_window.h) written out: through the helper hipcc lays this kernel's address arithmetic out
                // differently and it runs about 1 % slower.  Keep the two in step.
                float ax = 0.f, ay = 0.f, q = 0.f, rr = 0.f;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy) {
                    const float wy = tap_count(gy, gy + dy, H);
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const float wgt = wy * tap_count(gx, gx + dx, W);
                        const float4 kf = coef[(ly + 1 + dy) * RW + lx + 1 + dx];
                        ax += wgt * kf.x;
                        ay += wgt * kf.y;
                        q += wgt * kf.z;
                        rr += wgt * kf.w;
                    }
                }
                const float xc = sx[(ly + 2) * SW + lx + 4], yc = sy[(ly + 2) * SW + lx + 4];
                const float diff = yc - xc, sg = sgn(diff);
                const float l1 = ssel[(ly + 1) * RW + lx + 1] == k ? (1.f - alpha) * gl * sg : 0.f;
                if (G) G[((int64_t)n * C + c) * plane + (int64_t)gy * W + gx] = in_scale * (ay + q * xc + rr * yc + l1);
                gt[r] += ax + q * yc + rr * xc - l1;
            }
        }
        if (g_tgt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gy = y0 + ly0 + r;
                if (gx < W && gy < H) g_tgt[((int64_t)n * C + c) * plane + (int64_t)gy * W + gx] = in_scale * gt[r];
            }
        }
    }
}

inline int64_t minreproj_blocks(int B, int H, int W) {
    const dim3 g = ssim_grid(B, H, W);
    return (int64_t)g.x * g.y * g.z;
}

// candidate pointers all present (K = V or 2V of them); 16-byte row staging needs every image 16-byte aligned
inline bool minreproj_ptrs(MinReprojPtrs &p, const float *tgt, const float *const *cands, int K, int W, int *vec) {
    uintptr_t bits = reinterpret_cast<uintptr_t>(tgt);
    for (int k = 0; k < MAX_K; ++k) {
        p.cand[k] = k < K ? cands[k] : nullptr;
        if (k < K && !cands[k]) return false;
        bits |= reinterpret_cast<uintptr_t>(p.cand[k]);
    }
    *vec = (W % 4 == 0 && (bits & 15) == 0) ? 1 : 0;
    return true;
}

}  // namespace

extern "C" {

int64_t dvf_minreproj_partials_floats(int B, int H, int W, int K) {
    if (B <= 0 || H <= 0 || W <= 0 || K < 1 || K > MAX_K) return 0;
    return minreproj_blocks(B, H, W) * (K + 2);      // one loss partial and K+1 integer counts per block
}

int dvf_minreproj_fwd(const float *tgt, const float *const *cands, int V, int auto_mask, float *loss_out, uint8_t *select,
                      int32_t *counts, float *partials, int B, int C, int H, int W, float in_scale, float alpha, float c1, float c2,
                      int accumulate, void *stream) {
    if (!tgt || !cands || !loss_out || !select || !counts || !partials || V < 1 || V > MAX_V || !image_shape_ok(B, C, H, W, 3))
        return DVF_ERR_INVALID_ARG;
    const int K = auto_mask ? 2 * V : V;
    MinReprojPtrs p = {};
    int vec = 0;
    if (!minreproj_ptrs(p, tgt, cands, K, W, &vec)) return DVF_ERR_INVALID_ARG;
    hipStream_t st = dvf_stream(stream);
    const int64_t nblk = minreproj_blocks(B, H, W);
    int *cnt_partials = reinterpret_cast<int *>(partials + nblk);
    minreproj_fwd_kernel<<<ssim_grid(B, H, W), NT, 0, st>>>(tgt, p, V, K, select, partials, cnt_partials, C, H, W, in_scale, alpha, c1,
                                                            c2, vec);
    DVF_LAUNCH_CHECK();
    const float scale = (float)(1.0 / ((double)B * C * H * W));
    minreproj_reduce_kernel<<<1, 256, 0, st>>>(partials, cnt_partials, nblk, K, scale, loss_out, counts, accumulate);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

int dvf_minreproj_bwd(const float *tgt, const float *const *cands, int V, int auto_mask, const uint8_t *select,
                      const float *grad_loss, float *g_tgt, float *const *g_warped, int B, int C, int H, int W, float in_scale,
                      float alpha, float c1, float c2, void *stream) {
    if (!tgt || !cands || !select || !grad_loss || V < 1 || V > MAX_V || !image_shape_ok(B, C, H, W, 3)) return DVF_ERR_INVALID_ARG;
    const int K = auto_mask ? 2 * V : V;
    MinReprojPtrs p = {};
    int vec = 0;
    if (!minreproj_ptrs(p, tgt, cands, K, W, &vec)) return DVF_ERR_INVALID_ARG;
    bool any = g_tgt != nullptr;
    for (int k = 0; k < V; ++k) {
        p.g[k] = g_warped ? g_warped[k] : nullptr;
        any |= p.g[k] != nullptr;
    }
    if (!any) return DVF_OK;
    const float inv_n = (float)(1.0 / ((double)B * C * H * W));
    minreproj_bwd_kernel<<<ssim_grid(B, H, W), NT, 0, dvf_stream(stream)>>>(tgt, p, V, K, select, grad_loss, g_tgt, C, H, W, in_scale,
                                                                            alpha, c1, c2, inv_n, vec);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

}  // extern "C"
