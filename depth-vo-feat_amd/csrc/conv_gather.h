// Register-staged gather-form convolution kernel (launched from conv.hip).
//
//  conv_gather_kernel   out[m][Y][X] = sum_r sum_taps W(m, r, tap) * in[r][iy][ix]      ("gather form")
//      GEMM view: M = output channels (MFMA rows, 32 per tile), N = 32 output pixels per tile (one pixel per
//      lane -> coalesced NCHW stores), K = (input channel pair) x taps.  The input patch (+halo) of CK channels
//      and the matching weight slab are staged in LDS once per chunk and re-used by every tap.
//      Used as: Conv2d forward (stride 1/2), Conv2d dgrad and ConvTranspose2d forward (the output parity classes
//      share one launch, so strided layers waste no MACs on zeros), ConvTranspose2d dgrad.  Virtual concat: up to 3
//      input segments are walked in place of torch.cat.
#pragma once
#include "dvf_common.h"
#include "conv_pipe.h"

namespace {

using dvfp::f32x16;
using dvfp::tensor_rsrc;
using dvfp::OOB;
using dvfp::bload;
using dvfp::store_tile;

struct ClassDev { int py, px, by, bx, TA, TB, OHc, OWc, tap0; };

struct GatherArgs {
    const float *in[DVF_MAX_SEGS];
    int segC[DVF_MAX_SEGS];
    int nseg;
    const float *w;
    int w_mode;          // 0: w[((m_base+m)*Rtot + r)*KK + tap]   1: w[(r*Mtot + m_base+m)*KK + tap]
    int Mtot, Rtot, KK, m_base, M;
    const float *bias;   // indexed by m (already offset by the caller) or NULL
    float *out;          // [N, M, OH, OW]
    int N, IH, IW, OH, OW;
    int OS, IS;          // output pixel (oy*OS+py, ox*OS+px); input pixel (oy*IS+by+ta, ox*IS+bx+tb)
    int ncls;            // output-parity classes handled by this launch (blockIdx.z % ncls)
    ClassDev cls[4];
    int act;
    float alpha, beta;
    int KS, NCH, out_mode, dbg;          // out_mode: dvfp::OutMode (conv_epilogue.h)
    int64_t ws_slice;
    int lsw, lsh, TGX, BW, BH, tilesX, tilesY;
    int PSmax, Tmax, WD; // LDS carve: patch CK*PSmax | weights Tmax*CK*COTP | wdec WD | tapB Tmax | inv 64
    int tapmap[52];      // class c uses tapmap[cls[c].tap0 + t]: class tap -> tap index of the stored kernel
    const float *mask;   // (dgrad) ReLU backward of the producing layer, out = (mask > 0) ? v : 0, same shape as out: applied here when OUT_FUSED, else by finish_output
};

// MT x 32 output channels, 4*NT tiles of 32 pixels per block, CK = 2*CKH reduction channels per LDS chunk.
template <int MT, int NT, int CKH>
__global__ __launch_bounds__(256) void conv_gather_kernel(const GatherArgs a) {
    constexpr int CK = 2 * CKH, COTP = 32 * MT + 1;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *patch = smem;                                   // [CK][PH][RS] (IS==2: columns split by parity)
    float *wl = smem + CK * a.PSmax;                       // [T][CK][COTP]
    int *wdec = reinterpret_cast<int *>(wl + a.Tmax * CK * COTP);   // weight run element -> LDS offset
    int *tapB = wdec + a.WD;                               // class tap -> patch offset
    int *inv = tapB + a.Tmax;                              // stored tap -> class tap
    const int tid = threadIdx.x, lane = tid & 63, nl = lane & 31, kh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // wave-uniform: row/column bookkeeping stays scalar
    const int zc = blockIdx.z % a.ncls, zr = blockIdx.z / a.ncls;
    const int n = zr / a.KS, ks = zr - n * a.KS;
    const ClassDev c = a.cls[zc];
    const int tX = blockIdx.x % a.tilesX, tY = blockIdx.x / a.tilesX;
    const int oy0 = tY * a.BH, ox0 = tX * a.BW;
    if (oy0 >= c.OHc || ox0 >= c.OWc) return;              // tile outside this (smaller) class: whole block exits
    const int m0 = blockIdx.y * (32 * MT);
    const int SW = 1 << a.lsw, SH = 1 << a.lsh;
    const int pxl = nl & (SW - 1), pyl = nl >> a.lsw;
    const int T = c.TA * c.TB;
    const int PH = (a.BH - 1) * a.IS + c.TA, PW = (a.BW - 1) * a.IS + c.TB, PWH = (PW + 1) >> 1;
    const int RS = (a.IS == 2) ? 2 * PWH : PW, PS = PH * RS;

    // ---- one-time tables
    for (int e = tid; e < 64; e += 256) inv[e] = -1;
    __syncthreads();
    for (int t = tid; t < T; t += 256) {
        inv[a.tapmap[c.tap0 + t]] = t;
        const int ta = t / c.TB, tb = t - ta * c.TB;
        tapB[t] = ta * RS + ((a.IS == 2) ? ((tb & 1) * PWH + (tb >> 1)) : tb);
    }
    __syncthreads();
    {
        const int nE = (a.w_mode == 0 ? CK : 32 * MT) * a.KK;
        for (int e = tid; e < nE; e += 256) {
            const int hi = e / a.KK, t = inv[e - hi * a.KK];        // hi = r (mode 0) or m (mode 1)
            int d = -1;
            if (t >= 0) d = (hi << 24) | (a.w_mode == 0 ? (t * CK + hi) * COTP : t * CK * COTP + hi);
            wdec[e] = d;
        }
    }

    int boff[NT], opy[NT], opx[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int q = wave * NT + i, tx = q % a.TGX, ty = q / a.TGX;
        opy[i] = ty * SH + pyl;
        opx[i] = tx * SW + pxl;
        boff[i] = kh * PS + (opy[i] * a.IS) * RS + opx[i];
    }
    f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][i][r] = 0.f;

    const int iy0 = oy0 * a.IS + c.by, ix0 = ox0 * a.IS + c.bx;
    // lane-invariant column part of the patch staging: byte offset inside a row (or OOB) and LDS column (or -1)
    const bool npass2 = PW > 64;
    unsigned pcol_off[2];
    int pcol_dst[2];
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        const int cc = lane + 64 * ps, ix = ix0 + cc;
        pcol_off[ps] = (cc < PW && ix >= 0 && ix < a.IW) ? ((unsigned)ix << 2) : OOB;
        pcol_dst[ps] = (cc < PW) ? ((a.IS == 2) ? ((cc & 1) * PWH + (cc >> 1)) : cc) : -1;
    }
    const __amdgpu_buffer_rsrc_t rs_w = tensor_rsrc(a.w);
    const int g_begin = (int)(((int64_t)a.NCH * ks) / a.KS), g_end = (int)(((int64_t)a.NCH * (ks + 1)) / a.KS);
    int seg = 0, seg_first = 0, r_seg = 0;     // r_seg: index of the segment's first channel in the concat
    for (int g = g_begin; g < g_end; ++g) {
        while (true) {
            const int nchs = (a.segC[seg] + CK - 1) / CK;
            if (g < seg_first + nchs) break;
            seg_first += nchs;
            r_seg += a.segC[seg];
            ++seg;
        }
        const int c0 = (g - seg_first) * CK;                  // first channel of the chunk inside its segment
        const int nch = min(CK, a.segC[seg] - c0);            // valid channels in this chunk
        __syncthreads();                                      // previous chunk fully consumed (and tables visible)
        // ---- stage the input patch.  Row bookkeeping is scalar and incremental (no divisions); everything that
        // depends on the lane (column offset, column validity, LDS column) was computed once before the chunk loop.
        // 8 independent buffer loads are issued before the 8 LDS stores.
        if (!DVF_DBG(a, 1)) {
            const __amdgpu_buffer_rsrc_t rs_in = tensor_rsrc(a.in[seg]);
            const unsigned cb = (unsigned)((n * a.segC[seg] + c0) * a.IH * a.IW) << 2;      // chunk base, bytes
            int ci = 0, r = wave;                              // this wave's next row (ci, r); rows advance by 4
            while (r >= PH) { r -= PH; ++ci; }
            while (ci < CK) {
                float v[8][2];
                int dsts[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    dsts[k] = -1;
                    if (ci < CK) {
                        const int iy = iy0 + r;
                        const bool rowok = (ci < nch) & (iy >= 0) & (iy < a.IH);
                        const unsigned soff = cb + ((unsigned)((ci * a.IH + iy) * a.IW) << 2);
                        dsts[k] = ci * PS + r * RS;
                        v[k][0] = bload(rs_in, rowok ? pcol_off[0] : OOB, rowok ? soff : 0u);
                        if (npass2) v[k][1] = bload(rs_in, rowok ? pcol_off[1] : OOB, rowok ? soff : 0u);
                        r += 4;
                        while (r >= PH) { r -= PH; ++ci; }
                    }
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (dsts[k] >= 0) {
                        if (pcol_dst[0] >= 0) patch[dsts[k] + pcol_dst[0]] = v[k][0];
                        if (npass2 && pcol_dst[1] >= 0) patch[dsts[k] + pcol_dst[1]] = v[k][1];
                    }
                }
            }
        }
        // ---- stage the weight slab wl[(t*CK + r)*COTP + m]: lanes walk the contiguous run of the stored tensor
        // (coalesced), wdec[] maps a run position to its LDS slot; row bases are scalar 32-bit offsets.
        if (!DVF_DBG(a, 2)) {
            const int r0 = r_seg + c0;                        // reduction index of the chunk's first channel
            if (a.w_mode == 0) {
                const int nE = CK * a.KK;
                const unsigned wb = (unsigned)(((a.m_base + m0) * a.Rtot + r0) * a.KK) << 2;
                const unsigned rowstep = (unsigned)(a.Rtot * a.KK) << 2;
                for (int e = lane; e < nE; e += 64) {
                    const int d = wdec[e];
                    const bool use = d >= 0;
                    const unsigned voff = (use && ((d >> 24) < nch)) ? ((unsigned)e << 2) : OOB;
                    const int off = d & 0xFFFFFF;
                    float v[8 * MT];
#pragma unroll
                    for (int k = 0; k < 8 * MT; ++k) {
                        const int m = wave + 4 * k;
                        const bool mok = m0 + m < a.M;
                        v[k] = bload(rs_w, mok ? voff : OOB, mok ? wb + (unsigned)m * rowstep : 0u);
                    }
                    if (use) {
#pragma unroll
                        for (int k = 0; k < 8 * MT; ++k) wl[off + wave + 4 * k] = v[k];
                    }
                }
            } else {
                const int nE = 32 * MT * a.KK;
                const unsigned wb = (unsigned)((r0 * a.Mtot + a.m_base + m0) * a.KK) << 2;
                const unsigned rowstep = (unsigned)(a.Mtot * a.KK) << 2;
                constexpr int RK = (CK + 3) / 4;                // reduction rows per wave
                for (int e0 = lane; e0 < nE; e0 += 256) {
                    int d[4];
                    float v[4][RK];
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const int e = e0 + 64 * jj;
                        d[jj] = (e < nE) ? wdec[e] : -1;
                    }
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const int e = e0 + 64 * jj;
                        const unsigned voff = ((d[jj] >= 0) && (m0 + (d[jj] >> 24) < a.M)) ? ((unsigned)e << 2) : OOB;
#pragma unroll
                        for (int k = 0; k < RK; ++k) {
                            const int rr = wave + 4 * k;
                            const bool rok = rr < nch;
                            v[jj][k] = bload(rs_w, rok ? voff : OOB, rok ? wb + (unsigned)rr * rowstep : 0u);
                        }
                    }
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        if (d[jj] < 0) continue;
#pragma unroll
                        for (int k = 0; k < RK; ++k) {
                            const int rr = wave + 4 * k;
                            if (rr < CK) wl[(d[jj] & 0xFFFFFF) + rr * COTP] = v[jj][k];
                        }
                    }
                }
            }
        }
        __syncthreads();
        // ---- MFMA: per tap, all CKH channel pairs; the next tap's fragments are fetched before this tap's MFMAs
        if (!DVF_DBG(a, 4)) {
            float af[2][CKH][MT], bf[2][CKH][NT];
            auto load = [&](auto bufc, int t) {
                constexpr int buf = decltype(bufc)::value;
                const int tb_off = tapB[t];
                const int wo = (t * CK + kh) * COTP + nl;
#pragma unroll
                for (int cp = 0; cp < CKH; ++cp) {
#pragma unroll
                    for (int m = 0; m < MT; ++m) af[buf][cp][m] = wl[wo + cp * 2 * COTP + m * 32];
#pragma unroll
                    for (int i = 0; i < NT; ++i) bf[buf][cp][i] = patch[boff[i] + tb_off + cp * 2 * PS];
                }
            };
            auto mma = [&](auto bufc) {
                constexpr int buf = decltype(bufc)::value;
#pragma unroll
                for (int cp = 0; cp < CKH; ++cp)
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int i = 0; i < NT; ++i)
                            acc[m][i] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[buf][cp][m], bf[buf][cp][i], acc[m][i], 0, 0, 0);
            };
            using B0 = std::integral_constant<int, 0>;
            using B1 = std::integral_constant<int, 1>;
            load(B0{}, 0);
            for (int t = 0; t < T; t += 2) {
                if (t + 1 < T) load(B1{}, t + 1);
                mma(B0{});
                if (t + 1 < T) {
                    if (t + 2 < T) load(B0{}, t + 2);
                    mma(B1{});
                }
            }
        }
    }
    // ---- epilogue (store_tile, conv_epilogue.h): one image per block, the bias comes from global memory
    const int64_t HWo = (int64_t)a.OH * a.OW;
    store_tile<MT, NT>(
        acc, a.out + (a.out_mode == dvfp::OUT_WS ? (int64_t)ks * a.ws_slice : 0), a.mask, a.out_mode, a.act, a.alpha, a.beta, m0, kh, a.M, HWo,
        [&](int i, int64_t &off) __attribute__((always_inline)) {
            const int oy = oy0 + opy[i], ox = ox0 + opx[i];
            const int Y = oy * a.OS + c.py, X = ox * a.OS + c.px;
            off = ((int64_t)n * a.M + m0 + 4 * kh) * HWo + (int64_t)Y * a.OW + X;
            return (oy < c.OHc) && (ox < c.OWc) && (Y < a.OH) && (X < a.OW);
        },
        [&](int ml) __attribute__((always_inline)) {
            const int mm = m0 + ml + 4 * kh;
            return (a.bias && mm < a.M) ? a.bias[mm] : 0.f;
        });
}

}  // namespace
