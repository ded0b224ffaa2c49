// Opt-in regulariser: first-order, edge-aware smoothness of the MEAN-NORMALISED disparity (monodepth2 form).  The reference
// has no such term -- its smoothness is second-order on depth (loss_functions.py:23-41) or the Caffe graph's un-normalised
// edge-aware one (paper_losses.hip) -- so there is NO reference call site, parity is UNPINNED and tests/normsmooth_ref.py is
// the definition.  Per image b, with I = fl(in_scale * img) [B,C,H,W] and disp [B,1,H,W]:
//   m_b  = mean over (H,W) of disp_b                        n = disp / (m_b + eps)
//   wx   = exp(-mean_c |I(y,x) - I(y,x+1)|)                 wy = exp(-mean_c |I(y,x) - I(y+1,x)|)
//   loss = weight * (mean(wx |n(y,x) - n(y,x+1)|) + mean(wy |n(y,x) - n(y+1,x)|))
// the two means running over B*H*(W-1) and B*(H-1)*W elements.  Only disp receives a gradient; d|v|/dv = 0 at v = 0.
//
// The mean couples every pixel of an image through one scalar, but with that scalar fixed the term is LINEAR in |delta disp|:
//   T_b  = Sx_b / (B H (W-1)) + Sy_b / (B (H-1) W),   Sx_b = sum wx |dx disp|,  Sy_b = sum wy |dy disp|
//   loss = weight * sum_b T_b / |m_b + eps|
// so neither direction needs a pass for the mean followed by a pass for the loss.
//
// Forward = ONE tile pass + one small finishing launch.
//   norm_smooth_fwd_kernel     one block owns a 64x16 pixel tile of one image (blocks never straddle images); every pixel owns
//                              its right and its lower difference; the block stores three partials: sum disp, Sx, Sy.
//   norm_smooth_finish_kernel  one block; per image the tile partials are added in a fixed order, stats[b] = (m_b + eps, T_b)
//                              is stored, then the images are added in index order into loss_out.  No atomics anywhere: the
//                              loss is bit-reproducible.
// Backward = ONE launch, GATHER form, no atomics.  Every pixel p collects from its up to four neighbours q
//   A_p = sum_q sign(disp_p - disp_q) * w(p,q) * (1/(B H (W-1)) for a horizontal pair, 1/(B (H-1) W) for a vertical one),
// the weights recomputed from the image (w is symmetric in its pair), and writes, with M = m_b + eps,
//   g_p = grad_loss * weight * (A_p / |M| - T_b / (M |M| H W))        (= A_p / M - T_b / (M^2 H W) for a positive mean)
// Every element of g_disp is written exactly once; nothing needs zeroing.
#include "dvf_common.h"

namespace {

constexpr int TW = 64, TH = 16, NT = 256, ROWS = TH / (NT / 64);   // 4 vertically adjacent pixels per thread

static inline dim3 ns_grid(int B, int H, int W) { return dim3((W + TW - 1) / TW, (H + TH - 1) / TH, B); }

// exp(-mean_c |I_p - I_q|) of the pixel pair at plane offsets p and q of one image.  CT: the channel count when it is known at
// compile time (1 and 3: the channel loop unrolls and its loads are issued together), 0 = read it from C.
template <int CT>
__device__ __forceinline__ float edge_weight(const float *__restrict__ I, int64_t plane, int C, int p, int q, float in_scale,
                                             float inv_c) {
    float s = 0.f;
    const int nc = CT ? CT : C;
#pragma unroll
    for (int c = 0; c < nc; ++c) s += fabsf(__fmul_rn(in_scale, I[c * plane + p]) - __fmul_rn(in_scale, I[c * plane + q]));
    return __expf(-s * inv_c);
}

template <int CT>
__global__ __launch_bounds__(NT) void norm_smooth_fwd_kernel(const float *__restrict__ disp, const float *__restrict__ img,
                                                             float *__restrict__ partials, int C, int H, int W, float in_scale) {
    __shared__ float red[3][NT / 64];
    const int n = blockIdx.z, gx = blockIdx.x * TW + (threadIdx.x & 63), gy0 = blockIdx.y * TH + (threadIdx.x >> 6) * ROWS;
    const int64_t plane = (int64_t)H * W;
    const float *D = disp + n * plane, *I = img + (int64_t)n * C * plane;
    const float inv_c = 1.f / (float)C;
    float sd = 0.f, sx = 0.f, sy = 0.f;
    if (gx < W) {
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            const int gy = gy0 + k;
            if (gy >= H) break;
            const int p = gy * W + gx;
            const float d = D[p];
            sd += d;
            if (gx + 1 < W) sx += edge_weight<CT>(I, plane, C, p, p + 1, in_scale, inv_c) * fabsf(d - D[p + 1]);
            if (gy + 1 < H) sy += edge_weight<CT>(I, plane, C, p, p + W, in_scale, inv_c) * fabsf(d - D[p + W]);
        }
    }
    sd = wave_sum(sd);
    sx = wave_sum(sx);
    sy = wave_sum(sy);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = sd;
        red[1][threadIdx.x >> 6] = sx;
        red[2][threadIdx.x >> 6] = sy;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int64_t blk = linear_block();
        const float *r = red[threadIdx.x];
        partials[blk * 3 + threadIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
    }
}

// partials [B][tiles][3] -> stats [B][2] = (m_b + eps, T_b), loss_out.  One block of 256 threads; wave w reduces images
// w, w + 4, ..., lane-strided over the tiles, then wave 0 adds T_b / |m_b + eps| lane-strided over the images.
__global__ __launch_bounds__(NT) void norm_smooth_finish_kernel(const float *partials, int B, int tiles, float inv_hw, float cx,
                                                                float cy, float eps, float weight, float *stats, float *loss_out,
                                                                int accumulate) {
    const int lane = threadIdx.x & 63;
    for (int b = threadIdx.x >> 6; b < B; b += NT / 64) {
        const float *P = partials + (int64_t)b * tiles * 3;
        float sd = 0.f, sx = 0.f, sy = 0.f;
        for (int i = lane; i < tiles; i += 64) {
            sd += P[i * 3];
            sx += P[i * 3 + 1];
            sy += P[i * 3 + 2];
        }
        sd = wave_sum(sd);
        sx = wave_sum(sx);
        sy = wave_sum(sy);
        if (lane == 0) {
            stats[b * 2] = sd * inv_hw + eps;
            stats[b * 2 + 1] = sx * cx + sy * cy;
        }
    }
    __syncthreads();   // the stats rows written above are read back by wave 0 of this same block
    if (threadIdx.x < 64) {
        float s = 0.f;
        for (int b = lane; b < B; b += 64) s += stats[b * 2 + 1] / fabsf(stats[b * 2]);
        s = wave_sum(s);
        if (lane == 0) {
            const float t = __fmul_rn(weight, s);   // (no contraction with the add below: accumulate adds the SAME loss)
            loss_out[0] = accumulate ? loss_out[0] + t : t;
        }
    }
}

template <int CT>
__global__ __launch_bounds__(NT) void norm_smooth_bwd_kernel(const float *__restrict__ disp, const float *__restrict__ img,
                                                             const float *__restrict__ stats, const float *__restrict__ grad_loss,
                                                             float *__restrict__ g_disp, int C, int H, int W, float in_scale,
                                                             float cx, float cy, float inv_hw, float weight) {
    const int n = blockIdx.z, gx = blockIdx.x * TW + (threadIdx.x & 63), gy0 = blockIdx.y * TH + (threadIdx.x >> 6) * ROWS;
    if (gx >= W) return;
    const int64_t plane = (int64_t)H * W;
    const float *D = disp + n * plane, *I = img + (int64_t)n * C * plane;
    const float inv_c = 1.f / (float)C;
    const float M = stats[n * 2], T = stats[n * 2 + 1];
    const float gl = grad_loss[0] * weight, ia = 1.f / fabsf(M);
    const float mean_term = T * inv_hw / M;        // (A_p - T / (M H W)) / |M|
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        const int gy = gy0 + k;
        if (gy >= H) break;
        const int p = gy * W + gx;
        const float d = D[p];
        float ax = 0.f, ay = 0.f;
        if (gx > 0) ax += sgn(d - D[p - 1]) * edge_weight<CT>(I, plane, C, p, p - 1, in_scale, inv_c);
        if (gx + 1 < W) ax += sgn(d - D[p + 1]) * edge_weight<CT>(I, plane, C, p, p + 1, in_scale, inv_c);
        if (gy > 0) ay += sgn(d - D[p - W]) * edge_weight<CT>(I, plane, C, p, p - W, in_scale, inv_c);
        if (gy + 1 < H) ay += sgn(d - D[p + W]) * edge_weight<CT>(I, plane, C, p, p + W, in_scale, inv_c);
        g_disp[n * plane + p] = gl * ((ax * cx + ay * cy) - mean_term) * ia;
    }
}

}  // namespace

extern "C" {

int64_t dvf_norm_smooth_partials_floats(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const dim3 g = ns_grid(B, H, W);
    return (int64_t)g.x * g.y * g.z * 3;
}

int dvf_norm_smooth_fwd(const float *disp, const float *img, float *loss_out, float *stats, float *partials, int B, int C, int H,
                        int W, float in_scale, float eps, float weight, int accumulate, void *stream) {
    if (!disp || !img || !loss_out || !stats || !partials || !image_shape_ok(B, C, H, W, 2)) return DVF_ERR_INVALID_ARG;
    hipStream_t st = dvf_stream(stream);
    const dim3 grid = ns_grid(B, H, W);
    if (C == 3) norm_smooth_fwd_kernel<3><<<grid, NT, 0, st>>>(disp, img, partials, C, H, W, in_scale);
    else if (C == 1) norm_smooth_fwd_kernel<1><<<grid, NT, 0, st>>>(disp, img, partials, C, H, W, in_scale);
    else norm_smooth_fwd_kernel<0><<<grid, NT, 0, st>>>(disp, img, partials, C, H, W, in_scale);
    DVF_LAUNCH_CHECK();
    const float cx = (float)(1.0 / ((double)B * H * (W - 1))), cy = (float)(1.0 / ((double)B * (H - 1) * W));
    norm_smooth_finish_kernel<<<1, NT, 0, st>>>(partials, B, (int)(grid.x * grid.y), (float)(1.0 / ((double)H * W)), cx, cy, eps,
                                                weight, stats, loss_out, accumulate);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

int dvf_norm_smooth_bwd(const float *disp, const float *img, const float *stats, const float *grad_loss, float *g_disp, int B,
                        int C, int H, int W, float in_scale, float eps, float weight, void *stream) {
    (void)eps;   // stats already holds m_b + eps; the parameter keeps the pair's signatures parallel
    if (!disp || !img || !stats || !grad_loss || !g_disp || !image_shape_ok(B, C, H, W, 2)) return DVF_ERR_INVALID_ARG;
    const float cx = (float)(1.0 / ((double)B * H * (W - 1))), cy = (float)(1.0 / ((double)B * (H - 1) * W));
    const float inv_hw = (float)(1.0 / ((double)H * W));
    const dim3 grid = ns_grid(B, H, W);
    hipStream_t st = dvf_stream(stream);
    if (C == 3) norm_smooth_bwd_kernel<3><<<grid, NT, 0, st>>>(disp, img, stats, grad_loss, g_disp, C, H, W, in_scale, cx, cy, inv_hw, weight);
    else if (C == 1) norm_smooth_bwd_kernel<1><<<grid, NT, 0, st>>>(disp, img, stats, grad_loss, g_disp, C, H, W, in_scale, cx, cy, inv_hw, weight);
    else norm_smooth_bwd_kernel<0><<<grid, NT, 0, st>>>(disp, img, stats, grad_loss, g_disp, C, H, W, in_scale, cx, cy, inv_hw, weight);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

}  // extern "C"
