// Device and host helpers shared by the 3x3-window appearance kernels (ssim_loss.hip, minreproj_loss.hip): the 64x16 tile
// geometry, plane staging with a reflected border, the window evaluation, and the gather backward: the ring windows' coefficients
// (ring_coef) and their reflected-tap-counted sum per pixel (ring_gather).
#pragma once
#include "dvf_common.h"

namespace {

constexpr int TW = 64, TH = 16, NT = 256;
constexpr int SW = 72;                 // LDS row stride: tile column 0 sits at float 4 of a row, so 16-byte row pieces stay aligned
constexpr int RW = TW + 2, RH = TH + 2;  // halo-1 ring of windows around the tile (backward)

// reflect an index that is at most n-1 outside [0, n) (n >= 3); anything farther out is clamped (those values are never used)
__device__ __forceinline__ int reflect_idx(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
    return min(max(i, 0), n - 1);
}

// Stage rows y0-HALO .. y0+TH+HALO-1, columns x0-HALO .. x0+TW+HALO-1 of one plane (border reflected) times in_scale.
template <int HALO>
__device__ __forceinline__ void stage_plane(float *__restrict__ dst, const float *__restrict__ src, int H, int W, int y0, int x0,
                                            float in_scale, int vec) {
    constexpr int ROWS = TH + 2 * HALO;
    for (int i = threadIdx.x; i < ROWS * (TW / 4); i += NT) {
        const int r = i / (TW / 4), c4 = (i % (TW / 4)) * 4;
        const float *row = src + (int64_t)reflect_idx(y0 - HALO + r, H) * W;
        const int gx = x0 + c4;
        float4 v;
        if (vec && gx + 3 < W) {
            v = *reinterpret_cast<const float4 *>(row + gx);
        } else {
            v.x = row[reflect_idx(gx, W)];
            v.y = row[reflect_idx(gx + 1, W)];
            v.z = row[reflect_idx(gx + 2, W)];
            v.w = row[reflect_idx(gx + 3, W)];
        }
        v.x = __fmul_rn(in_scale, v.x);
        v.y = __fmul_rn(in_scale, v.y);
        v.z = __fmul_rn(in_scale, v.z);
        v.w = __fmul_rn(in_scale, v.w);
        *reinterpret_cast<float4 *>(dst + r * SW + 4 + c4) = v;
    }
    for (int i = threadIdx.x; i < ROWS * 2 * HALO; i += NT) {
        const int r = i / (2 * HALO), k = i % (2 * HALO);
        const int lc = k < HALO ? k - HALO : TW + k - HALO;      // tile-relative column
        const float *row = src + (int64_t)reflect_idx(y0 - HALO + r, H) * W;
        dst[r * SW + 4 + lc] = __fmul_rn(in_scale, row[reflect_idx(x0 + lc, W)]);
    }
}

struct SsimWin { float mx, my, a1, a2, b1, b2, ssim, dssim, gate; };

// Window whose top-left tap is at LDS offset o.
__device__ __forceinline__ SsimWin ssim_window(const float *sx, const float *sy, int o, float c1, float c2) {
    float x[9], y[9], sumx = 0.f, sumy = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[3 * r + c] = sx[o + r * SW + c];
            y[3 * r + c] = sy[o + r * SW + c];
            sumx += x[3 * r + c];
            sumy += y[3 * r + c];
        }
    constexpr float ninth = 1.f / 9.f;
    SsimWin w;
    w.mx = sumx * ninth;
    w.my = sumy * ninth;
    float vx = 0.f, vy = 0.f, cxy = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const float dx = x[t] - w.mx, dy = y[t] - w.my;
        vx += dx * dx;
        vy += dy * dy;
        cxy += dx * dy;
    }
    w.a1 = 2.f * w.mx * w.my + c1;
    w.a2 = 2.f * (cxy * ninth) + c2;
    w.b1 = w.mx * w.mx + w.my * w.my + c1;
    w.b2 = (vx + vy) * ninth + c2;
    w.ssim = (w.a1 * w.a2) / (w.b1 * w.b2);
    const float d = 0.5f * (1.f - w.ssim);
    w.gate = (d >= 0.f && d <= 1.f) ? 1.f : 0.f;
    w.dssim = fminf(fmaxf(d, 0.f), 1.f);
    return w;
}

// how often window q (0 <= q < n) reads pixel p = q + d, |d| <= 1, through its three taps along one axis
__device__ __forceinline__ float tap_count(int p, int q, int n) {
    if (q < 0 || q >= n) return 0.f;
    return ((q == 0 && p == 1) || (q == n - 1 && p == n - 2)) ? 2.f : 1.f;
}

// Gather backward, first half.  Within a window d dssim / d y_j = Py + Q x_j + R y_j is affine in the tap's own values (for
// x: Px, with x and y swapped); returns (Px, Py, Q, R) times `weight` (and times alpha and the clamp gate of dssim).
__device__ __forceinline__ float4 ring_coef(SsimWin w, float alpha, float weight) {
    constexpr float ninth = 1.f / 9.f;
    const float ib = 1.f / (w.b1 * w.b2);
    const float Q = 2.f * ninth * w.a1 * ib;                        // d SSIM / d cxy * (1/9) ... per tap
    const float R = -2.f * ninth * w.ssim / w.b2;
    const float Px = ninth * (2.f * w.my * w.a2 * ib - 2.f * w.mx * w.ssim / w.b1) - Q * w.my - R * w.mx;
    const float Py = ninth * (2.f * w.mx * w.a2 * ib - 2.f * w.my * w.ssim / w.b1) - Q * w.mx - R * w.my;
    const float f = -0.5f * alpha * w.gate * weight;                // dssim = (1 - SSIM) / 2
    float4 k;        // by value in, field by field out: make_float4 over a reference changes the contraction into FMAs
    k.x = f * Px;
    k.y = f * Py;
    k.z = f * Q;
    k.w = f * R;
    return k;
}

// Second half: pixel (gy, gx), at (ly, lx) of the tile, sums the coefficients of the <= 9 ring windows that contain it; a
// window that reaches the pixel through the reflected border counts twice per axis.
__device__ __forceinline__ float4 ring_gather(const float4 *coef, int ly, int lx, int gy, int gx, int H, int W) {
    float ax = 0.f, ay = 0.f, q = 0.f, r = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const float wy = tap_count(gy, gy + dy, H);
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const float wgt = wy * tap_count(gx, gx + dx, W);
            const float4 k = coef[(ly + 1 + dy) * RW + lx + 1 + dx];
            ax += wgt * k.x;
            ay += wgt * k.y;
            q += wgt * k.z;
            r += wgt * k.w;
        }
    }
    return make_float4(ax, ay, q, r);
}

inline dim3 ssim_grid(int B, int H, int W) { return dim3((W + TW - 1) / TW, (H + TH - 1) / TH, B); }

inline int ssim_vec(const float *a, const float *b, int W) {
    return (W % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0) ? 1 : 0;
}

}  // namespace
