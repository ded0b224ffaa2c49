// What the convolution kernels share after their main loop: the output modes, the activation and the store loop of an
// MFMA accumulator tile (conv_pipe_kernel, conv_gather_kernel; the direct kernels of conv_head.hip use the activation).
#pragma once
#include "dvf_common.h"

namespace dvfp {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Where a launch's sums go (PipeArgs / GatherArgs::out_mode; the plan records carry the value).
enum OutMode {
    OUT_FUSED = 0,       // bias + activation (or the ReLU mask of a dgrad) in the epilogue
    OUT_ATOMIC = 1,      // atomicAdd into a zeroed output; bias, activation and mask follow in a finishing pass
    OUT_WS = 2           // K-split ks stores its plain partial tile at ks * ws_slice of the workspace; one pass reduces them
};

template <int ACT>
__device__ __forceinline__ float apply_act(float t, float alpha, float beta) {
    if constexpr (ACT == DVF_ACT_RELU) return fmaxf(t, 0.f);
    else if constexpr (ACT == DVF_ACT_SIGMOID_AFFINE) return alpha * (1.f / (1.f + expf(-t))) + beta;
    else return t;
}
__device__ __forceinline__ float apply_act(float v, int act, float alpha, float beta) {
    if (act == DVF_ACT_RELU) return apply_act<DVF_ACT_RELU>(v, alpha, beta);
    if (act == DVF_ACT_SIGMOID_AFFINE) return apply_act<DVF_ACT_SIGMOID_AFFINE>(v, alpha, beta);
    return v;
}

// Store the MT x NT accumulator tiles of a wave, D[row = channel][col = pixel]: accumulator register r of lane half kh
// (lanes 0-31 / 32-63) of tile m is channel row m*32 + (r&3) + 8*(r>>2) + 4*kh of the wave's channels m0 ...
//   out      the output, or this K-split's slice of the workspace (OUT_WS)
//   pix(i, off) -> the pixel of this lane in sub-tile i exists; off = element offset of (image, channel m0 + 4*kh, pixel)
//   bias_at(ml) -> bias of the lane's channel row ml (OUT_FUSED only)
// The output mode, the activation and "every channel of this wave exists" are launch constants: the store loop is
// instantiated per combination (evaluated per element they cost 30+ scalar branches, an inlined sigmoid and a dependent
// bias load in every one of the 16*MT*NT stores of a lane -- microseconds per block); rows are reached by scalar
// multiples of HW.  MODE 0-2: OutMode; 3: OUT_FUSED with the ReLU mask of a dgrad (no bias / activation of its own).
template <int MT, int NT, class Pix, class Bias>
__device__ __forceinline__ void store_tile(const f32x16 (&acc)[MT][NT], float *out, const float *mask, int out_mode, int act,
                                           float alpha, float beta, int m0, int kh, int M, int64_t HW, Pix pix, Bias bias_at) {
    auto store_all = [&](auto modec, auto actc, auto fullc) __attribute__((always_inline)) {
        constexpr int MODE = decltype(modec)::value, ACT = decltype(actc)::value;
        constexpr bool FULL = decltype(fullc)::value;
        float bv[MT][16];
        if constexpr (MODE == 0) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) bv[m][r] = bias_at(m * 32 + (r & 3) + 8 * (r >> 2));   // (all loads in flight together)
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            int64_t off;
            const bool pok = pix(i, off);
            float *pbase = out + off;
            float mk[MT][16];
            if constexpr (MODE == 3) {           // all mask loads of the tile first (no branch around them: invalid elements read element 0)
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int ml = m * 32 + (r & 3) + 8 * (r >> 2);
                        const bool ok = pok && (FULL || m0 + 4 * kh + ml < M);
                        mk[m][r] = mask[ok ? off + (int64_t)ml * HW : 0];
                    }
            }
            if (pok) {
#pragma unroll
                for (int m = 0; m < MT; ++m) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int ml = m * 32 + (r & 3) + 8 * (r >> 2);
                        if (FULL || m0 + 4 * kh + ml < M) {
                            float *op = pbase + (int64_t)ml * HW;          // (ml * HW: scalar)
                            const float v = acc[m][i][r];
                            if constexpr (MODE == 3) *op = mk[m][r] > 0.f ? v : 0.f;
                            else if constexpr (MODE == 0) *op = apply_act<ACT>(v + bv[m][r], alpha, beta);
                            else if constexpr (MODE == 1) atomicAdd(op, v);
                            else *op = v;
                        }
                    }
                }
            }
        }
    };
    using std::integral_constant;
    auto by_full = [&](auto modec, auto actc) __attribute__((always_inline)) {
        if (m0 + 32 * MT <= M) store_all(modec, actc, std::true_type{});
        else store_all(modec, actc, std::false_type{});
    };
    if (out_mode == OUT_FUSED && mask) by_full(integral_constant<int, 3>{}, integral_constant<int, DVF_ACT_NONE>{});
    else if (out_mode == OUT_WS) by_full(integral_constant<int, 2>{}, integral_constant<int, DVF_ACT_NONE>{});
    else if (out_mode == OUT_ATOMIC) by_full(integral_constant<int, 1>{}, integral_constant<int, DVF_ACT_NONE>{});
    else if (act == DVF_ACT_RELU) by_full(integral_constant<int, 0>{}, integral_constant<int, DVF_ACT_RELU>{});
    else if (act == DVF_ACT_SIGMOID_AFFINE) by_full(integral_constant<int, 0>{}, integral_constant<int, DVF_ACT_SIGMOID_AFFINE>{});
    else by_full(integral_constant<int, 0>{}, integral_constant<int, DVF_ACT_NONE>{});
}

}  // namespace dvfp
