// On-device training augmentation (build-side extension; tests/augment_ref.py is the definition): random horizontal flip,
// zoom-and-crop and a colour perturbation of every frame of a sample, with the matching change of the intrinsics and of the
// stereo pose.  One 12-float record per sample (include/dvf_hip.h) drives both kernels.
//
// augment_frames_kernel is a streaming kernel: it reads each source frame once (the 2x2 taps of neighbouring outputs share
// cache lines, zoom <= 1.15) and writes each destination frame once.  A block stays inside one (frame, sample, channel)
// plane, so the record is read through uniform loads; a thread produces 4 consecutive output pixels of a row and stores them
// as one 16-byte store where the address allows it.  The gamma is exp2(gamma * log2(n)) on the hardware log2 / exp2.
#include "dvf_common.h"

namespace {

constexpr int AUG_MAX_FRAMES = 8, AUG_REC = 12, AUG_MAX_BLOCKS = 2048;

struct AugFrames {
    const float *src[AUG_MAX_FRAMES];
    float *dst[AUG_MAX_FRAMES];
};

// Clamped source coordinate of one axis -> the two tap indices and the fraction.  fmaxf / fminf drop a NaN, so any record
// (even one the host validation would refuse) yields taps inside [0, n-1].
__device__ __forceinline__ void aug_taps(float pos, float scale, int n, int &i0, int &i1, float &frac) {
    float u = __fmaf_rn(pos, scale, -0.5f);
    u = fminf(fmaxf(u, 0.f), (float)(n - 1));
    const float f = floorf(u);
    i0 = (int)f;
    i1 = min(i0 + 1, n - 1);
    frac = u - f;
}

__global__ __launch_bounds__(256) void augment_frames_kernel(AugFrames fr, const float *__restrict__ params, int B, int C, int H,
                                                             int W, float value_max) {
    const int plane = blockIdx.y;                       // (frame, sample, channel)
    const int c = plane % C, b = (plane / C) % B, f = plane / (C * B);
    const float *rec = params + (int64_t)b * AUG_REC;
    const bool flip = rec[0] > 0.5f;
    const float xscale = (float)W / rec[1], yscale = (float)H / rec[2];
    const float ox = rec[3] + 0.5f, oy = rec[4] + 0.5f;
    const bool colour = rec[5] > 0.5f;
    const float gamma = rec[6], gain = rec[7] * rec[8 + c], inv_max = 1.f / value_max;
    const int64_t off = ((int64_t)b * C + c) * H * W;
    const float *__restrict__ src = fr.src[f] + off;
    float *__restrict__ dst = fr.dst[f] + off;
    const int gpr = (W + 3) >> 2;                       // groups of 4 output pixels per row
    // item = (row, group), walked with the grid's stride; one division per thread, then increments
    const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    const int dy = stride / gpr, dg = stride - dy * gpr;
    int y = first / gpr, g = first - y * gpr;
    for (; y < H; y += dy, g += dg) {
        if (g >= gpr) {                                 // (g < 2 gpr: at most one carry)
            g -= gpr;
            if (++y >= H) break;
        }
        const int x4 = g * 4;
        int y0, y1;
        float fy;
        aug_taps((float)y + oy, yscale, H, y0, y1, fy);
        const float *r0 = src + (int64_t)y0 * W, *r1 = src + (int64_t)y1 * W;
        float out[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = min(x4 + j, W - 1);           // (lanes past the row end recompute the last pixel and store nothing)
            int x0, x1;
            float fx;
            aug_taps((float)(flip ? W - 1 - x : x) + ox, xscale, W, x0, x1, fx);
            const float top = (1.f - fx) * r0[x0] + fx * r0[x1];
            const float bot = (1.f - fx) * r1[x0] + fx * r1[x1];
            float v = (1.f - fy) * top + fy * bot;
            if (colour) {                               // uniform over the block
                float n = v * inv_max;
                n = __builtin_amdgcn_exp2f(gamma * __builtin_amdgcn_logf(n));   // n^gamma; log2(0) = -inf -> 0
                v = value_max * fminf(fmaxf(n * gain, 0.f), 1.f);
            }
            out[j] = v;
        }
        float *o = dst + (int64_t)y * W + x4;
        if (x4 + 4 <= W && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
            *reinterpret_cast<float4 *>(o) = make_float4(out[0], out[1], out[2], out[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x4 + j < W) o[j] = out[j];
        }
    }
}

// One thread per sample: K' = A K M, Kinv' = M Kinv A^-1 (A^-1 in closed form), the two stereo-pose sign rules.  Everything
// is read before anything is written, so every output may alias its input.
__global__ __launch_bounds__(64) void augment_geometry_kernel(const float *params, const float *K, const float *Kinv, const float *T_tr,
                                                              const float *T_se3, float *K_out, float *Kinv_out, float *T_tr_out,
                                                              float *T_se3_out, int B, int W, int H) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const float *rec = params + (int64_t)b * AUG_REC;
    const bool flip = rec[0] > 0.5f;
    const float sx = rec[1] / (float)W, sy = rec[2] / (float)H;
    const float cxo = 0.5f * (sx - 1.f) - rec[3], cyo = 0.5f * (sy - 1.f) - rec[4];
    const float a = flip ? -sx : sx, c = flip ? (float)(W - 1) - cxo : cxo;
    const float m = flip ? -1.f : 1.f;
    float k[9], ki[9], tr[6], se[6];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        k[i] = K[b * 9 + i];
        ki[i] = Kinv[b * 9 + i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        tr[i] = T_tr[b * 6 + i];
        se[i] = T_se3[b * 6 + i];
    }
    const float ia = 1.f / a, isy = 1.f / sy;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float mj = j == 0 ? m : 1.f;              // (A K) M: column 0 changes sign under flip
        K_out[b * 9 + j] = (a * k[j] + c * k[6 + j]) * mj;
        K_out[b * 9 + 3 + j] = (sy * k[3 + j] + cyo * k[6 + j]) * mj;
        K_out[b * 9 + 6 + j] = k[6 + j] * mj;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float mi = i == 0 ? m : 1.f;              // M (Kinv A^-1): row 0 changes sign under flip
        Kinv_out[b * 9 + 3 * i] = ki[3 * i] * ia * mi;
        Kinv_out[b * 9 + 3 * i + 1] = ki[3 * i + 1] * isy * mi;
        Kinv_out[b * 9 + 3 * i + 2] = (ki[3 * i + 2] - c * ia * ki[3 * i] - cyo * isy * ki[3 * i + 1]) * mi;
    }
    // conjugation by M = diag(-1, 1, 1): (t, r) and (w, u) change sign where an odd number of x indices is involved
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const bool neg_tr = i == 0 || i == 4 || i == 5, neg_se = i == 1 || i == 2 || i == 3;
        T_tr_out[b * 6 + i] = flip && neg_tr ? -tr[i] : tr[i];
        T_se3_out[b * 6 + i] = flip && neg_se ? -se[i] : se[i];
    }
}

}  // namespace

extern "C" {

int dvf_augment_frames(const float *const *src, float *const *dst, int F, const float *params, int B, int C, int H, int W,
                       float value_max, void *stream) {
    if (!src || !dst || !params || F < 1 || F > AUG_MAX_FRAMES || B <= 0 || C != 3 || H <= 0 || W <= 0 || !(value_max > 0.f))
        return DVF_ERR_INVALID_ARG;
    const int64_t planes = (int64_t)F * B * C, n = (int64_t)B * C * H * W;
    if (planes > 65535 || (int64_t)H * W >= ((int64_t)1 << 30)) return DVF_ERR_INVALID_ARG;
    AugFrames fr = {};
    for (int i = 0; i < F; ++i) {
        if (!src[i] || !dst[i]) return DVF_ERR_INVALID_ARG;
        fr.src[i] = src[i];
        fr.dst[i] = dst[i];
    }
    // the gather reads the whole source frame: no destination may overlap a source, or another destination
    for (int i = 0; i < F; ++i)
        for (int j = 0; j < F; ++j) {
            const uintptr_t d = (uintptr_t)dst[i], s = (uintptr_t)src[j], e = (uintptr_t)dst[j], len = (uintptr_t)n * sizeof(float);
            if (d < s + len && s < d + len) return DVF_ERR_INVALID_ARG;
            if (i != j && d < e + len && e < d + len) return DVF_ERR_INVALID_ARG;
        }
    const int64_t items = (int64_t)H * ((W + 3) >> 2);
    int64_t gx = (items + 255) / 256;
    const int64_t cap = AUG_MAX_BLOCKS / planes > 0 ? AUG_MAX_BLOCKS / planes : 1;
    if (gx > cap) gx = cap;
    augment_frames_kernel<<<dim3((unsigned)gx, (unsigned)planes), 256, 0, dvf_stream(stream)>>>(fr, params, B, C, H, W, value_max);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

int dvf_augment_geometry(const float *params, const float *K, const float *Kinv, const float *T_tr, const float *T_se3,
                         float *K_out, float *Kinv_out, float *T_tr_out, float *T_se3_out, int B, int W, int H, void *stream) {
    if (!params || !K || !Kinv || !T_tr || !T_se3 || !K_out || !Kinv_out || !T_tr_out || !T_se3_out || B <= 0 || W <= 0 || H <= 0)
        return DVF_ERR_INVALID_ARG;
    augment_geometry_kernel<<<cdiv(B, 64), 64, 0, dvf_stream(stream)>>>(params, K, Kinv, T_tr, T_se3, K_out, Kinv_out, T_tr_out,
                                                                        T_se3_out, B, W, H);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

}  // extern "C"
