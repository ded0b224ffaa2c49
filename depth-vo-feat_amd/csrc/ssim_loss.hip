// Opt-in appearance term: alpha * DSSIM + (1 - alpha) * L1 between a target image x and an already warped reference y
// (monodepth2 form; the reference has no SSIM -- SURVEY.md preamble #1 -- so there is no reference call site and parity is
// UNPINNED; tests/ check this kernel pair against a torch restatement in fp64).  Definition, per image n and channel c, with
// x = fl(in_scale * tgt), y = fl(in_scale * warped):
//   3x3 window, uniform weights 1/9, REFLECTION border (index -1 -> 1, H -> H-2; same for W):
//     mx, my = window means;  vx = mean((x - mx)^2), vy = mean((y - my)^2), cxy = mean((x - mx)(y - my))   (centred form)
//   SSIM  = ((2 mx my + c1)(2 cxy + c2)) / ((mx^2 + my^2 + c1)(vx + vy + c2))
//   dssim = clamp((1 - SSIM) / 2, 0, 1)                       (derivative 0 outside the clamp range)
//   term  = alpha * dssim + (1 - alpha) * |x - y|
//   valid = 1 - prod_c [y_c == 0] at the centre pixel (the reference's exact-zero mask; no gradient)
//   loss  = sum(term * valid * m) / (B C H W)                 (m: optional explainability mask, receives a gradient)
//
// Forward: one block owns a 64x16 pixel tile of one image; per channel it stages x and y with halo 1 in LDS, each thread
// evaluates 4 vertically adjacent windows, one partial per block, fixed-order reduce: the loss is bit-reproducible.
// Backward: GATHER form, no atomics.  Within window q, d dssim_q / d y_j = Py_q + Q_q x_j + R_q y_j is affine in the tap's
// own values (same for x with Px_q and x, y swapped), so per channel the block stages halo 2, computes the four
// coefficients (times alpha * valid_q * m_q * gate_q * grad / N) of the halo-1 ring of windows once into LDS, and every pixel
// sums the <= 9 windows that contain it -- a window that reaches the pixel through the reflected border counts twice per
// axis -- plus its own L1 sign term.  Every output element is written exactly once.
#include "ssim_window.h"

namespace {

__global__ __launch_bounds__(NT) void ssim_fwd_kernel(const float *tgt, const float *warped, const float *mask,
                                                      int64_t mask_batch_stride, float *partials, int C, int H, int W,
                                                      float in_scale, float alpha, float c1, float c2, int vec) {
    __shared__ __attribute__((aligned(16))) float sx[(TH + 2) * SW];
    __shared__ __attribute__((aligned(16))) float sy[(TH + 2) * SW];
    __shared__ float red[NT / 64];
    const int n = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int lx = threadIdx.x & 63, ly0 = (threadIdx.x >> 6) * 4, gx = x0 + lx;
    const int64_t plane = (int64_t)H * W;
    const float *X = tgt + (int64_t)n * C * plane, *Y = warped + (int64_t)n * C * plane;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    bool nonzero[4] = {false, false, false, false};
    for (int c = 0; c < C; ++c) {
        __syncthreads();
        stage_plane<1>(sx, X + c * plane, H, W, y0, x0, in_scale, vec);
        stage_plane<1>(sy, Y + c * plane, H, W, y0, x0, in_scale, vec);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (gx >= W || y0 + ly0 + k >= H) continue;
            const int o = (ly0 + k) * SW + lx + 3;
            const SsimWin w = ssim_window(sx, sy, o, c1, c2);
            const float xc = sx[o + SW + 1], yc = sy[o + SW + 1];
            acc[k] += alpha * w.dssim + (1.f - alpha) * fabsf(xc - yc);
            nonzero[k] |= (yc != 0.f);
        }
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int gy = y0 + ly0 + k;
        if (gx < W && gy < H && nonzero[k])
            s += mask ? acc[k] * mask[(int64_t)n * mask_batch_stride + (int64_t)gy * W + gx] : acc[k];
    }
    s = block_sum(s, threadIdx.x >> 6, red);
    if (threadIdx.x == 0) partials[linear_block()] = s;
}

__global__ __launch_bounds__(NT) void ssim_bwd_kernel(const float *tgt, const float *warped, const float *mask,
                                                      int64_t mask_batch_stride, const float *grad_loss, float *g_warped,
                                                      float *g_tgt, float *g_mask, int C, int H, int W, float in_scale, float alpha,
                                                      float c1, float c2, float inv_n, int vec) {
    __shared__ __attribute__((aligned(16))) float sx[(TH + 4) * SW];
    __shared__ __attribute__((aligned(16))) float sy[(TH + 4) * SW];
    __shared__ __attribute__((aligned(16))) float4 coef[RH * RW];   // (Px, Py, Q, R) of each ring window, weighted
    __shared__ float sd[RH * RW];                                   // alpha * dssim of each ring window
    __shared__ float swt[RH * RW];                                  // valid * m * grad_loss / N of each ring pixel (0 outside the image)
    const int n = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int lx = threadIdx.x & 63, ly0 = (threadIdx.x >> 6) * 4, gx = x0 + lx;
    const int64_t plane = (int64_t)H * W;
    const float *X = tgt + (int64_t)n * C * plane, *Y = warped + (int64_t)n * C * plane;
    const float gl = grad_loss[0] * inv_n;

    for (int i = threadIdx.x; i < RH * RW; i += NT) {
        const int qy = y0 - 1 + i / RW, qx = x0 - 1 + i % RW;
        float wt = 0.f;
        if (qy >= 0 && qy < H && qx >= 0 && qx < W) {
            const int64_t p = (int64_t)qy * W + qx;
            bool nz = false;
            for (int c = 0; c < C; ++c) nz |= (__fmul_rn(in_scale, Y[c * plane + p]) != 0.f);
            if (nz) wt = mask ? gl * mask[(int64_t)n * mask_batch_stride + p] : gl;
        }
        swt[i] = wt;
    }
    float gm[4] = {0.f, 0.f, 0.f, 0.f};
    bool nonzero[4] = {false, false, false, false};
    for (int c = 0; c < C; ++c) {
        __syncthreads();
        stage_plane<2>(sx, X + c * plane, H, W, y0, x0, in_scale, vec);
        stage_plane<2>(sy, Y + c * plane, H, W, y0, x0, in_scale, vec);
        __syncthreads();
        for (int i = threadIdx.x; i < RH * RW; i += NT) {
            const int ry = i / RW, rx = i % RW;
            const float wt = swt[i];
            float4 k = make_float4(0.f, 0.f, 0.f, 0.f);
            float d = 0.f;
            if (y0 - 1 + ry >= 0 && y0 - 1 + ry < H && x0 - 1 + rx >= 0 && x0 - 1 + rx < W) {
                const SsimWin w = ssim_window(sx, sy, ry * SW + rx + 2, c1, c2);
                k = ring_coef(w, alpha, wt);
                d = alpha * w.dssim;
            }
            coef[i] = k;
            sd[i] = d;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ly = ly0 + r, gy = y0 + ly;
            if (gx >= W || gy >= H) continue;
            const float4 s = ring_gather(coef, ly, lx, gy, gx, H, W);
            const float xc = sx[(ly + 2) * SW + lx + 4], yc = sy[(ly + 2) * SW + lx + 4];
            const float diff = yc - xc;
            const float l1 = (1.f - alpha) * swt[(ly + 1) * RW + lx + 1] * sgn(diff);
            const int64_t o = ((int64_t)n * C + c) * plane + (int64_t)gy * W + gx;
            if (g_warped) g_warped[o] = in_scale * (s.y + s.z * xc + s.w * yc + l1);
            if (g_tgt) g_tgt[o] = in_scale * (s.x + s.z * yc + s.w * xc - l1);
            gm[r] += sd[(ly + 1) * RW + lx + 1] + (1.f - alpha) * fabsf(diff);
            nonzero[r] |= (yc != 0.f);
        }
    }
    if (g_mask) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ly = ly0 + r, gy = y0 + ly;
            if (gx >= W || gy >= H) continue;
            g_mask[(int64_t)n * mask_batch_stride + (int64_t)gy * W + gx] = nonzero[r] ? gl * gm[r] : 0.f;
        }
    }
}

}  // namespace

extern "C" {

int64_t dvf_ssim_partials_floats(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const dim3 g = ssim_grid(B, H, W);
    return (int64_t)g.x * g.y * g.z;
}

int dvf_ssim_loss_fwd(const float *tgt, const float *warped, const float *mask, int64_t mask_batch_stride, float *loss_out,
                      float *partials, int B, int C, int H, int W, float in_scale, float alpha, float c1, float c2, int accumulate,
                      void *stream) {
    if (!tgt || !warped || !loss_out || !partials || !image_shape_ok(B, C, H, W, 3) || (mask && mask_batch_stride < (int64_t)H * W))
        return DVF_ERR_INVALID_ARG;
    hipStream_t st = dvf_stream(stream);
    const dim3 grid = ssim_grid(B, H, W);
    ssim_fwd_kernel<<<grid, NT, 0, st>>>(tgt, warped, mask, mask_batch_stride, partials, C, H, W, in_scale, alpha, c1, c2,
                                         ssim_vec(tgt, warped, W));
    DVF_LAUNCH_CHECK();
    const float scale = (float)(1.0 / ((double)B * C * H * W));
    return dvf_sum_partials(partials, (int64_t)grid.x * grid.y * grid.z, scale, loss_out, accumulate, st);
}

int dvf_ssim_loss_bwd(const float *tgt, const float *warped, const float *mask, int64_t mask_batch_stride, const float *grad_loss,
                      float *g_warped, float *g_tgt, float *g_mask, int B, int C, int H, int W, float in_scale, float alpha,
                      float c1, float c2, void *stream) {
    if (!tgt || !warped || !grad_loss || !image_shape_ok(B, C, H, W, 3) ||
        ((mask || g_mask) && mask_batch_stride < (int64_t)H * W))
        return DVF_ERR_INVALID_ARG;
    if (!g_warped && !g_tgt && !g_mask) return DVF_OK;
    const float inv_n = (float)(1.0 / ((double)B * C * H * W));
    ssim_bwd_kernel<<<ssim_grid(B, H, W), NT, 0, dvf_stream(stream)>>>(tgt, warped, mask, mask_batch_stride, grad_loss, g_warped,
                                                                       g_tgt, g_mask, C, H, W, in_scale, alpha, c1, c2, inv_n,
                                                                       ssim_vec(tgt, warped, W));
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

}  // extern "C"
