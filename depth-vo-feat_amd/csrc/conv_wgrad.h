// Register-staged weight-gradient kernel and its planner (launched from conv.hip for what wgrad_pipe refuses).
//
//  conv_wgrad_kernel    G[m][c][tap] += sum_pixels P[m][pix] * Q[c][pix*S + tap - pad]
//      GEMM view: M = P channels, N = 32 (c, tap) columns per tile, K = pixel pairs.  Conv2d: P = dL/dpre,
//      Q = input;  ConvTranspose2d: P = input, Q = dL/dpre.  Each block keeps its G tile in MFMA accumulators
//      across many pixel tiles and adds it to global memory once.
#pragma once
#include "dvf_common.h"
#include "conv_pipe.h"
#include "conv_op.h"

namespace {

using dvfp::f32x16;
using dvfp::tensor_rsrc;
using dvfp::OOB;
using dvfp::bload;

struct WgradArgs {
    const float *P;      // [N, PCtot, GH, GW]; rows m_base .. m_base+M-1 are used
    const float *Q;      // [N, QCtot, QH, QW]; channels q_base .. q_base+Cq-1 are used
    float *G;            // G[(m_base_g + m) * g_mstride + (g_cbase + c) * KK + tap]
    int PCtot, m_base, M, QCtot, q_base, Cq;
    int64_t g_mstride;
    int g_mbase, g_cbase, KK, KH, KW;
    int N, GH, GW, QH, QW, S, pad;
    int CK, BH, lnp, tilesX, tilesY, PSPLIT;
    int PHq, PWq, PWH, RS, PS, COTP;
    int vp;              // P tile loaded in 16-byte lanes (GW % 4 == 0, 16-byte aligned base)
    int dbg;             // ablation switches (-DDVF_TUNING builds): 1 no Q loads, 2 no P loads, 4 no MFMA, 8 no atomic epilogue, 16 no LDS stores
};

constexpr int WG_BW = 32;

template <int MT, int NTW, bool PF>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const WgradArgs a) {
    constexpr int COTP = 32 * MT + 1;              // padded row of the transposed P tile (compile-time: immediate offsets)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *qp = smem;                               // [CK][PHq][RS]
    float *pl = smem + a.CK * a.PS;                 // [BH*32 pixels][COTP]
    const int tid = threadIdx.x, lane = tid & 63, nl = lane & 31, kh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.x * (32 * MT);
    const int c0 = blockIdx.y * a.CK;
    const int nch = min(a.CK, a.Cq - c0);
    const int T = a.KH * a.KW;
    const int ncols = nch * T;
    // this lane's columns: tile u of this wave covers columns (wave*NTW+u)*32 + nl
    int loff[NTW], gcol[NTW];
#pragma unroll
    for (int u = 0; u < NTW; ++u) {
        const int j = (wave * NTW + u) * 32 + nl;
        if (j < ncols) {
            const int cj = j / T, tj = j - cj * T, ta = tj / a.KW, tb = tj - ta * a.KW;
            const int toff = (a.S == 2) ? ((tb & 1) * a.PWH + (tb >> 1)) : tb;
            loff[u] = cj * a.PS + ta * a.RS + toff;
            gcol[u] = (a.g_cbase + c0 + cj) * a.KK + tj;
        } else {
            loff[u] = 0;
            gcol[u] = -1;
        }
    }
    f32x16 acc[MT][NTW];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int u = 0; u < NTW; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][u][r] = 0.f;

    const __amdgpu_buffer_rsrc_t rs_q = tensor_rsrc(a.Q), rs_p = tensor_rsrc(a.P);
    const bool qpass2 = a.PWq > 64;
    int qcol_dst[2];                               // lane-invariant LDS column of the Q patch (or -1)
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        const int cc = lane + 64 * ps;
        qcol_dst[ps] = (cc < a.PWq) ? ((a.S == 2) ? ((cc & 1) * a.PWH + (cc >> 1)) : cc) : -1;
    }
    const int ntiles = a.N * a.tilesX * a.tilesY;
    // Staging is split into ISSUE (global loads into registers) and STORE (registers -> LDS).  With PF the loads of
    // tile t+1 are issued right before the MFMA phase of tile t and stored after it, so their latency hides behind the
    // MFMAs (the register budget allows it when a wave stages at most WG_QMAX patch rows in one pass).
    constexpr int WG_QMAX = 24, WG_PMAX = 16 * MT;
    float qreg[WG_QMAX], preg[WG_PMAX];
    const int npairs = a.BH >> 1, ptotal = 32 * MT * npairs;
    auto tile_origin = [&](int tile, int &n, int &gy0, int &gx0) {
        n = tile / (a.tilesX * a.tilesY);
        const int rem = tile - n * (a.tilesX * a.tilesY);
        const int tY = rem / a.tilesX, tX = rem - tY * a.tilesX;
        gy0 = tY * a.BH;
        gx0 = tX * WG_BW;
    };
    auto issue_tile = [&](int tile) {
        int n, gy0, gx0;
        tile_origin(tile, n, gy0, gx0);
        if (!DVF_DBG(a, 1)) {   // Q patch rows wave, wave+4, ...: one 64-lane load per row (single pass: PWq <= 64)
            const int qy0 = gy0 * a.S - a.pad, qx0 = gx0 * a.S - a.pad;
            const unsigned cb = (unsigned)((n * a.QCtot + a.q_base + c0) * a.QH * a.QW) << 2;
            const int ix = qx0 + lane;
            const unsigned qoff = (lane < a.PWq && ix >= 0 && ix < a.QW) ? ((unsigned)ix << 2) : OOB;
            int ci = 0, r = wave;
            while (r >= a.PHq) { r -= a.PHq; ++ci; }
#pragma unroll
            for (int k = 0; k < WG_QMAX; ++k) {
                if (ci < a.CK) {
                    const int iy = qy0 + r;
                    const bool rowok = (ci < nch) & (iy >= 0) & (iy < a.QH);
                    const unsigned soff = cb + ((unsigned)((ci * a.QH + iy) * a.QW) << 2);
                    qreg[k] = bload(rs_q, rowok ? qoff : OOB, rowok ? soff : 0u);
                    r += 4;
                    while (r >= a.PHq) { r -= a.PHq; ++ci; }
                }
            }
        }
        if (DVF_DBG(a, 2)) {
        } else if (a.vp) {
            // P tile in 16-byte lanes: instruction k of this wave = image row (k' % BH) of the 8 channels 8*(k'/BH)..+7,
            // k' = wave + 4k; lane = (channel seg = lane >> 3, pixel group q = lane & 7 -> pixels 4q..4q+3).  4x fewer
            // vector-memory instructions than one float per lane: this kernel is bound by their issue rate.
            const int seg = lane >> 3, q = lane & 7;
            const unsigned plane = (unsigned)(a.GH * a.GW) << 2;
            const bool colok = gx0 + 4 * q < a.GW;                       // (GW % 4 == 0: a group is all in or all out)
            const unsigned pb = (unsigned)((n * a.PCtot + a.m_base + m0) * a.GH * a.GW) << 2;
            const unsigned lane_off = (unsigned)seg * plane + ((unsigned)(gx0 + 4 * q) << 2);
            const int nitems = 4 * MT * a.BH;
#pragma unroll
            for (int k = 0; k < WG_PMAX / 4; ++k) {
                const int it = wave + 4 * k, mg = it / a.BH, row = it - mg * a.BH;
                const int gy = gy0 + row;
                const bool ok = (it < nitems) & colok & (gy < a.GH) & (m0 + mg * 8 + seg < a.M);
                const unsigned soff = pb + (unsigned)(mg * 8) * plane + ((unsigned)(gy * a.GW) << 2);
                typedef float f4 __attribute__((ext_vector_type(4)));
                const f4 v4 = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs_p, ok ? lane_off : OOB, ok ? soff : 0u, 0));
                preg[4 * k + 0] = v4.x; preg[4 * k + 1] = v4.y; preg[4 * k + 2] = v4.z; preg[4 * k + 3] = v4.w;
            }
        } else {   // P tile: item idx = (channel m, row pair rp); half-wave = one row of 32 pixels
            const int px = lane & 31, prow = lane >> 5;
            const bool colok = gx0 + px < a.GW;
            const unsigned pb = (unsigned)((n * a.PCtot + a.m_base + m0) * a.GH * a.GW) << 2;
#pragma unroll
            for (int k = 0; k < WG_PMAX; ++k) {
                const int idx = wave + 4 * k;
                const int m = idx >> a.lnp, rp = idx - (m << a.lnp);
                const int gy = gy0 + rp * 2 + prow;
                const bool mok = (idx < ptotal) & (m0 + m < a.M);
                const unsigned voff = (colok && gy < a.GH) ? ((unsigned)(gy * a.GW + gx0 + px) << 2) : OOB;
                preg[k] = bload(rs_p, mok ? voff : OOB, mok ? pb + ((unsigned)(m * a.GH * a.GW) << 2) : 0u);
            }
        }
    };
    auto store_tile = [&]() {
        if (DVF_DBG(a, 16)) return;
        {
            int ci = 0, r = wave;
            while (r >= a.PHq) { r -= a.PHq; ++ci; }
#pragma unroll
            for (int k = 0; k < WG_QMAX; ++k) {
                if (ci < a.CK) {
                    if (qcol_dst[0] >= 0) qp[ci * a.PS + r * a.RS + qcol_dst[0]] = qreg[k];
                    r += 4;
                    while (r >= a.PHq) { r -= a.PHq; ++ci; }
                }
            }
        }
        if (a.vp) {
            const int seg = lane >> 3, q = lane & 7;
            const int nitems = 4 * MT * a.BH;
#pragma unroll
            for (int k = 0; k < WG_PMAX / 4; ++k) {
                const int it = wave + 4 * k, mg = it / a.BH, row = it - mg * a.BH;
                if (it < nitems) {
                    float *dst = pl + (row * WG_BW + 4 * q) * COTP + mg * 8 + seg;     // bank = 4q + j + seg: conflict-free
#pragma unroll
                    for (int j = 0; j < 4; ++j) dst[j * COTP] = preg[4 * k + j];
                }
            }
        } else {
            const int px = lane & 31, prow = lane >> 5;
#pragma unroll
            for (int k = 0; k < WG_PMAX; ++k) {
                const int idx = wave + 4 * k;
                const int m = idx >> a.lnp, rp = idx - (m << a.lnp);
                if (idx < ptotal) pl[((rp * 2 + prow) * WG_BW + px) * COTP + m] = preg[k];
            }
        }
    };
    if (PF && blockIdx.z < ntiles) issue_tile(blockIdx.z);
    for (int tile = blockIdx.z; tile < ntiles; tile += a.PSPLIT) {
        int n, gy0, gx0;
        tile_origin(tile, n, gy0, gx0);
        __syncthreads();
        if (PF) {
            store_tile();
        } else {
        // ---- stage Q patch: scalar incremental row bookkeeping, lane-invariant column part, buffer loads (zero fill)
        {
            const int qy0 = gy0 * a.S - a.pad, qx0 = gx0 * a.S - a.pad;
            const unsigned cb = (unsigned)((n * a.QCtot + a.q_base + c0) * a.QH * a.QW) << 2;
            unsigned qcol_off[2];
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
                const int cc = lane + 64 * ps, ix = qx0 + cc;
                qcol_off[ps] = (cc < a.PWq && ix >= 0 && ix < a.QW) ? ((unsigned)ix << 2) : OOB;
            }
            int ci = 0, r = wave;
            while (r >= a.PHq) { r -= a.PHq; ++ci; }
            while (ci < a.CK) {
                float v[8][2];
                int dsts[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    dsts[k] = -1;
                    if (ci < a.CK) {
                        const int iy = qy0 + r;
                        const bool rowok = (ci < nch) & (iy >= 0) & (iy < a.QH);
                        const unsigned soff = cb + ((unsigned)((ci * a.QH + iy) * a.QW) << 2);
                        dsts[k] = ci * a.PS + r * a.RS;
                        v[k][0] = bload(rs_q, rowok ? qcol_off[0] : OOB, rowok ? soff : 0u);
                        if (qpass2) v[k][1] = bload(rs_q, rowok ? qcol_off[1] : OOB, rowok ? soff : 0u);
                        r += 4;
                        while (r >= a.PHq) { r -= a.PHq; ++ci; }
                    }
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (dsts[k] >= 0) {
                        if (qcol_dst[0] >= 0) qp[dsts[k] + qcol_dst[0]] = v[k][0];
                        if (qpass2 && qcol_dst[1] >= 0) qp[dsts[k] + qcol_dst[1]] = v[k][1];
                    }
                }
            }
        }
        // ---- stage P tile transposed: pl[pixel][m]; half-wave = one row of 32 pixels; 8 buffer loads per batch
        {
            const int npairs = a.BH >> 1;          // row pairs per channel
            const int px = lane & 31, prow = lane >> 5;
            const int total = 32 * MT * npairs;
            const bool colok = gx0 + px < a.GW;
            const unsigned pb = (unsigned)((n * a.PCtot + a.m_base + m0) * a.GH * a.GW) << 2;
            for (int ib = wave; ib < total; ib += 32) {
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int idx = ib + 4 * k;
                    const int m = idx >> a.lnp, rp = idx - (m << a.lnp);
                    const int gy = gy0 + rp * 2 + prow;
                    const bool mok = (idx < total) & (m0 + m < a.M);
                    const unsigned voff = (colok && gy < a.GH) ? ((unsigned)(gy * a.GW + gx0 + px) << 2) : OOB;
                    v[k] = bload(rs_p, mok ? voff : OOB, mok ? pb + ((unsigned)(m * a.GH * a.GW) << 2) : 0u);
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int idx = ib + 4 * k;
                    const int m = idx >> a.lnp, rp = idx - (m << a.lnp);
                    if (idx < total) pl[((rp * 2 + prow) * WG_BW + px) * COTP + m] = v[k];
                }
            }
        }
        }
        __syncthreads();
        if (PF && tile + a.PSPLIT < ntiles) issue_tile(tile + a.PSPLIT);     // in flight during the MFMA phase
        // ---- MFMA over pixel pairs: groups of 4 steps, the next group's fragments are fetched first
        {
            float af[2][4][MT], bf[2][4][NTW];
            // one VALU add per group and operand (lane part + scalar group part); steps and m-tiles are immediates.
            // (a VALU instruction between MFMAs costs 6-8 cycles of matrix-pipe time, LDS and scalar ones none)
            const float *a_lane = pl + kh * COTP + nl;
            const float *b_lane[NTW];
#pragma unroll
            for (int u = 0; u < NTW; ++u) b_lane[u] = qp + loff[u] + kh;
            auto load = [&](auto bufc, int py, int px0) {
                constexpr int buf = decltype(bufc)::value;
                const float *ag = a_lane + (py * WG_BW + px0) * COTP;
                const int qo = (py * a.S) * a.RS + px0;
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                    for (int m = 0; m < MT; ++m) af[buf][s4][m] = ag[2 * s4 * COTP + m * 32];
#pragma unroll
                for (int u = 0; u < NTW; ++u) {
                    const float *bg = b_lane[u] + qo;
#pragma unroll
                    for (int s4 = 0; s4 < 4; ++s4) bf[buf][s4][u] = bg[2 * s4];
                }
            };
            auto mma = [&](auto bufc) {
                constexpr int buf = decltype(bufc)::value;
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int u = 0; u < NTW; ++u)
                            acc[m][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[buf][s4][m], bf[buf][s4][u], acc[m][u], 0, 0, 0);
            };
            using B0 = std::integral_constant<int, 0>;
            using B1 = std::integral_constant<int, 1>;
            const int ngroups = DVF_DBG(a, 4) ? 0 : a.BH * 4;          // 32 pixels per row = 16 steps = 4 groups of 4 steps
            load(B0{}, 0, 0);
            for (int gq = 0; gq < ngroups; gq += 2) {
                load(B1{}, (gq + 1) >> 2, ((gq + 1) & 3) * 8);
                mma(B0{});
                if (gq + 2 < ngroups) load(B0{}, (gq + 2) >> 2, ((gq + 2) & 3) * 8);
                mma(B1{});
            }
        }
    }
    // ---- add the G tile: row = P channel, col = (c, tap)
    if (DVF_DBG(a, 8)) {                                   // (keep the accumulators alive)
        float s = 0.f;
#pragma unroll
        for (int u = 0; u < NTW; ++u)
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) s += acc[m][u][r];
        if (s == 1.2345e-30f) a.G[0] = s;
        return;
    }
#pragma unroll
    for (int u = 0; u < NTW; ++u) {
        if (gcol[u] < 0) continue;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int mm = m0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                if (mm < a.M) atomicAdd(a.G + (int64_t)(a.g_mbase + mm) * a.g_mstride + gcol[u], acc[m][u][r]);
            }
    }
}

// ---------------------------------------------------------------------------------------- host planning
struct WgradRegPlan { int MT, NTW; bool pf; size_t lds; dim3 grid; };

// Plan conv_wgrad_kernel for the roles, geometry and operands in `a`: fills its tiling fields.
int plan_wgrad_reg(WgradArgs &a, WgradRegPlan &pl) {
    const int KK = a.KK, MT = a.M > 32 ? 2 : 1;
    // column tiles per wave: two when the kernel is large, or when that lets fewer channel chunks (each of which
    // re-reads the whole P tensor) cover the segment
    static const int ntw_mode = dvf_tune("DVF_WG_NTW2") ? atoi(dvf_tune("DVF_WG_NTW2")) : 0;     // tuning knob
    int NTW = KK >= 25 ? 2 : 1;
    if (NTW == 1 && KK <= 128) {
        const int n1 = cdiv(a.Cq, 128 / KK), n2 = cdiv(a.Cq, 256 / KK);
        if ((ntw_mode == 1 && n2 == 1 && n1 > 1) || (ntw_mode == 2 && n2 < n1) || (ntw_mode == 3 && n2 < n1 && a.Cq * KK <= 1024))
            NTW = 2;
    }
    int CK = (128 * NTW) / KK;
    if (CK < 1) CK = 1;
    if (CK > a.Cq) CK = a.Cq;
    a.BH = a.GH <= 2 ? 2 : 4;
    a.lnp = ilog2(a.BH >> 1);
    a.tilesX = cdiv(a.GW, WG_BW);
    a.tilesY = cdiv(a.GH, a.BH);
    a.PHq = (a.BH - 1) * a.S + a.KH;
    a.PWq = (WG_BW - 1) * a.S + a.KW;
    a.PWH = (a.PWq + 1) / 2;
    a.RS = (a.S == 2) ? 2 * a.PWH : a.PWq;
    a.PS = a.PHq * a.RS;
    a.COTP = 32 * MT + 1;
    // the block's LDS (Q patch + transposed P tile) may take the whole 64 KiB a block can address with immediate
    // offsets: two blocks per CU, but as many patch channels per block as fit -- every channel chunk re-reads the
    // whole P tensor, and fewer chunks beat a third resident block (swept 36..64 KB on cfg 2: 44 KB 9.02 ms/step,
    // 52 KB 8.57, 56 KB 8.47, 64 KB 8.43)
    static const size_t wg_lds_cap = (dvf_tune("DVF_WG_LDS_KB") ? atoi(dvf_tune("DVF_WG_LDS_KB")) : 64) * 1024;
    while (CK > 1 && ((size_t)CK * a.PS + (size_t)a.BH * WG_BW * a.COTP) * 4 > wg_lds_cap) --CK;
    a.CK = CK;
    const int mtiles = cdiv(a.M, 32 * MT), cchunks = cdiv(a.Cq, CK);
    const int ntiles = a.N * a.tilesX * a.tilesY;
    static const int wg_target = dvf_tune("DVF_WG_BLOCKS") ? atoi(dvf_tune("DVF_WG_BLOCKS")) : 512;    // one round of 2 blocks per CU (swept on cfg 2: 512..2048)
    int psplit = wg_target / (mtiles * cchunks);
    if (psplit < 1) psplit = 1;
    if (psplit > ntiles) psplit = ntiles;
    if (psplit > 65535 || cchunks > 65535) return DVF_ERR_UNSUPPORTED;
    a.PSPLIT = psplit;
    const size_t lds = ((size_t)CK * a.PS + (size_t)a.BH * WG_BW * a.COTP) * 4;
    if (lds > 80 * 1024) return DVF_ERR_UNSUPPORTED;
    {   // more than the default 64 KiB of dynamic LDS needs the per-function opt-in (once per process)
        static const bool raised = [] {
            const void *fns[] = {(const void *)&conv_wgrad_kernel<2, 2, true>,  (const void *)&conv_wgrad_kernel<2, 1, true>,
                                 (const void *)&conv_wgrad_kernel<1, 2, true>,  (const void *)&conv_wgrad_kernel<1, 1, true>,
                                 (const void *)&conv_wgrad_kernel<2, 2, false>, (const void *)&conv_wgrad_kernel<2, 1, false>,
                                 (const void *)&conv_wgrad_kernel<1, 2, false>, (const void *)&conv_wgrad_kernel<1, 1, false>};
            bool ok = true;
            for (const void *f : fns)
                ok = ok && hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024) == hipSuccess;
            return ok;
        }();
        if (!raised && lds > 64 * 1024) return DVF_ERR_UNSUPPORTED;
    }
    if ((int64_t)a.N * a.PCtot * a.GH * a.GW * 4 >= ((int64_t)1 << 31) - 16 ||
        (int64_t)a.N * a.QCtot * a.QH * a.QW * 4 >= ((int64_t)1 << 31) - 16)
        return DVF_ERR_UNSUPPORTED;             // 32-bit byte offsets inside the kernel
    // register prefetch of the next tile when a wave's share of the Q patch fits the register budget (one pass)
    static const bool no_pf = dvf_tune("DVF_WG_NOPF") != nullptr;
    const bool pf = !no_pf && a.PWq <= 64 && cdiv(CK * a.PHq, 4) <= 24 && 8 * MT * (a.BH >> 1) <= 16 * MT;
    static const bool no_vp = dvf_tune("DVF_WG_NOVP") != nullptr;
    a.vp = (pf && !no_vp && a.GW % 4 == 0 && (reinterpret_cast<uintptr_t>(a.P) & 15) == 0) ? 1 : 0;
    pl = WgradRegPlan{MT, NTW, pf, lds, dim3(mtiles, cchunks, psplit)};
    return DVF_OK;
}

int launch_wgrad_reg(WgradArgs a, const WgradRegPlan &pl, hipStream_t st) {
    if (const char *e = dvf_tune("DVF_WG_DBG")) a.dbg = atoi(e);
    dvf_note_wgrad_reg(pl.MT, pl.NTW, pl.pf, a.CK, a.BH, a.PSPLIT, a.vp, a.S, (int)pl.lds, a.KK);
    const int MT = pl.MT, NTW = pl.NTW;
    if (pl.pf) {
        if (MT == 2 && NTW == 2) conv_wgrad_kernel<2, 2, true><<<pl.grid, 256, pl.lds, st>>>(a);
        else if (MT == 2) conv_wgrad_kernel<2, 1, true><<<pl.grid, 256, pl.lds, st>>>(a);
        else if (NTW == 2) conv_wgrad_kernel<1, 2, true><<<pl.grid, 256, pl.lds, st>>>(a);
        else conv_wgrad_kernel<1, 1, true><<<pl.grid, 256, pl.lds, st>>>(a);
    } else {
        if (MT == 2 && NTW == 2) conv_wgrad_kernel<2, 2, false><<<pl.grid, 256, pl.lds, st>>>(a);
        else if (MT == 2) conv_wgrad_kernel<2, 1, false><<<pl.grid, 256, pl.lds, st>>>(a);
        else if (NTW == 2) conv_wgrad_kernel<1, 2, false><<<pl.grid, 256, pl.lds, st>>>(a);
        else conv_wgrad_kernel<1, 1, false><<<pl.grid, 256, pl.lds, st>>>(a);
    }
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

}  // namespace
