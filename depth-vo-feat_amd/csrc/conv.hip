// fp32 MFMA convolutions for gfx950 (v_mfma_f32_32x32x2_f32: exact fp32, bit-identical to an fmaf chain, so the 1e-4
// parity bound holds without any reduced-precision path): host side and C entry points of the convolution family.
//
// Every op is described once (conv_op.h: a forward, or the dgrad of one input segment), planned by a pure function of
// its kernel family and launched from the plan:
//   conv_pipe_kernel    conv_pipe.h / conv_pipe_host.h   pipelined gather form over pre-packed weights
//   conv_gather_kernel  conv_gather.h                    register-staged gather form over the stored weights
//   wgrad_pipe          wgrad_pipe.h / wgrad_pipe.hip    pipelined weight gradient
//   conv_wgrad_kernel   conv_wgrad.h                     register-staged weight gradient (what wgrad_pipe refuses)
//   direct kernels      conv_head.h / conv_head.hip      1-4 channel heads, thin stride-2 transposed convolutions
// Size queries call the planners only.
//
// Layouts are the reference's (NCHW activations, OIHW / IOHW weights): nothing is repacked between steps.
#include "dvf_common.h"
#include "conv_op.h"
#include "conv_pipe_host.h"
#include "conv_gather.h"
#include "conv_wgrad.h"
#include "wgrad_pipe.h"

namespace {

// dpre = dY * act'(Y) and dbias[c] += sum dpre  (one pass; dbias zeroed by the caller side of the ABI)
__device__ __forceinline__ float act_grad(float g, float yv, int act, float alpha, float beta) {
    if (act == DVF_ACT_RELU) return (yv > 0.f) ? g : 0.f;
    if (act == DVF_ACT_SIGMOID_AFFINE) {
        const float sg = (yv - beta) / alpha;               // sigmoid value
        return g * alpha * sg * (1.f - sg);
    }
    return g;
}

// dpre = dy * act'(y) and dbias[c] += sum(dpre) in one pass.  VEC: 16-byte lanes (HW % 4 == 0), 4 independent loads in
// flight per thread; one atomic per block.
// part != NULL: the block's sum goes to part[c * (N * chunks) + n * chunks + chunk] instead of an atomic on dbias[c]
// (bias_finish_kernel adds them in index order: run-to-run deterministic).
template <bool VEC>
__global__ __launch_bounds__(256) void act_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ y,
                                                      float *__restrict__ dpre, float *dbias, int C, int HW, int act,
                                                      float alpha, float beta, int chunks, float *part = nullptr, int nper = 0) {
    __shared__ float red[4];
    const int plane = blockIdx.x / chunks, chunk = blockIdx.x - plane * chunks;
    const int c = plane % C;
    const int64_t base = (int64_t)plane * HW;
    float s = 0.f;
    if (VEC) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        const int HW4 = HW >> 2, per = (HW4 + chunks - 1) / chunks;
        const int beg = chunk * per, end = min(HW4, beg + per);
        const f4 *dy4 = reinterpret_cast<const f4 *>(dy + base), *y4 = reinterpret_cast<const f4 *>(y ? y + base : dy + base);
        f4 *o4 = reinterpret_cast<f4 *>(dpre ? dpre + base : nullptr);
        for (int i0 = beg + threadIdx.x; i0 < end; i0 += 1024) {
            f4 g[4], yv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = i0 + 256 * k;
                if (i < end) { g[k] = dy4[i]; yv[k] = (act != DVF_ACT_NONE) ? y4[i] : g[k]; }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = i0 + 256 * k;
                if (i < end) {
                    f4 r;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { r[e] = act_grad(g[k][e], yv[k][e], act, alpha, beta); s += r[e]; }
                    if (dpre) o4[i] = r;
                }
            }
        }
    } else {
        const int per = (HW + chunks - 1) / chunks;
        const int beg = chunk * per, end = min(HW, beg + per);
        for (int i = beg + threadIdx.x; i < end; i += 256) {
            const float g = act_grad(dy[base + i], (act != DVF_ACT_NONE) ? y[base + i] : 0.f, act, alpha, beta);
            if (dpre) dpre[base + i] = g;
            s += g;
        }
    }
    if (dbias) {
        s = wave_sum(s);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            const float t = (red[0] + red[1]) + (red[2] + red[3]);
            if (part) part[(int64_t)c * nper + (plane / C) * chunks + chunk] = t;
            else atomicAdd(&dbias[c], t);
        }
    }
}

// dbias[c] += sum(dy[:, c]) alone (no activation, no dpre to write: the pass behind the weight gradient of a transposed
// layer).  A pure stream: the block reads its stretch of one (n, c) plane with eight independent 16-byte loads per thread
// and trip and no bounds test, then at most two trips of four clamped loads.  What bounds it besides the stream is the
// tail of float atomics: the 16 channels of a 64-byte line of dbias share one memory-side adder, ~15 ns per atomic
// (1664 blocks of the 16-channel full-resolution layer: 25 us), so the grid is a few hundred blocks (bias_sum_chunks) of up
// to 1024 threads, which keep as many bytes in flight as four times the blocks of 256 would.
// part != NULL: the block's sum goes to part[c * nper + n * chunks + chunk] (bias_finish_kernel adds them in index order).
template <bool VEC>
__global__ __launch_bounds__(1024) void bias_sum_kernel(const float *__restrict__ dy, float *dbias, int C, int HW, int chunks,
                                                        float *part, int nper) {
    __shared__ float red[16];
    constexpr int U = 8, UT = 4;
    typedef typename std::conditional<VEC, float __attribute__((ext_vector_type(4))), float>::type V;
    const int T = blockDim.x;
    const int plane = blockIdx.x / chunks, chunk = blockIdx.x - plane * chunks;
    const int c = plane % C;
    const int E = VEC ? HW >> 2 : HW, per = (E + chunks - 1) / chunks;      // elements (16-byte or 4-byte) of the plane, per block
    const int beg = chunk * per, n = min(E, beg + per) - beg;
    const V *p = reinterpret_cast<const V *>(dy + (int64_t)plane * HW) + beg;
    const V zero = {};
    V a0 = zero, a1 = zero;
    int i = threadIdx.x;
    for (; i + T * (U - 1) < n; i += T * U) {
        V g[U];
#pragma unroll
        for (int k = 0; k < U; ++k) g[k] = p[i + T * k];
#pragma unroll
        for (int k = 0; k < U; k += 2) { a0 += g[k]; a1 += g[k + 1]; }
    }
    for (; i < n; i += T * UT) {                 // (n > 0 here) loads clamped to the last element, masked when added
        V g[UT];
#pragma unroll
        for (int k = 0; k < UT; ++k) g[k] = p[min(i + T * k, n - 1)];
#pragma unroll
        for (int k = 0; k < UT; ++k) a0 += (i + T * k < n) ? g[k] : zero;
    }
    a0 += a1;
    float s;
    if constexpr (VEC) s = (a0[0] + a0[1]) + (a0[2] + a0[3]);
    else s = a0;
    s = wave_sum(s);
    if (T > 64) {
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            s = red[0];
            for (int w = 1; w < (T >> 6); ++w) s += red[w];
        }
    }
    if (threadIdx.x == 0) {
        if (part) part[(int64_t)c * nper + (plane / C) * chunks + chunk] = s;
        else atomicAdd(&dbias[c], s);
    }
}

// dbias[c] += part[c][0 .. n) summed in a fixed order (64 strided lane sums, then a fixed tree); one block per channel
__global__ __launch_bounds__(64) void bias_finish_kernel(const float *__restrict__ part, float *dbias, int n) {
    const float *p = part + (int64_t)blockIdx.x * n;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) s += p[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) dbias[blockIdx.x] += s;
}

// ------------------------------------------------------------------------------------- gather route
struct TilePlan { int lsw, lsh, TGX, TGY, NT; };

// pick the 32-pixel tile shape and the arrangement of a block's tiles that waste the fewest MFMA columns
TilePlan plan_tiles(int OHc, int OWc, int NT, int maxBW = 64) {
    TilePlan best{5, 0, 1, 4 * NT, NT};
    double best_cost = 1e30;
    for (int lsw = 5; lsw >= 0; --lsw) {
        const int lsh = 5 - lsw, SW = 1 << lsw, SH = 1 << lsh;
        for (int TGX = 1; TGX <= 4 * NT; TGX *= 2) {
            const int TGY = 4 * NT / TGX, BW = TGX * SW, BH = TGY * SH;
            if (BW > maxBW) continue;
            const double cov = (double)cdiv(OWc, BW) * BW * cdiv(OHc, BH) * BH;
            // small preference for wide tiles (coalesced stores) and compact patches
            const double cost = cov * (1.0 + 0.02 * lsh) + 1e-3 * (BW + BH);
            if (cost < best_cost) { best_cost = cost; best = TilePlan{lsw, lsh, TGX, TGY, NT}; }
        }
    }
    return best;
}

struct GatherPlan {
    GatherArgs a;            // geometry and tiling; the operands are set at launch
    int MT, NT, CKH;
    size_t lds;
    dim3 grid;
    int64_t ws_floats;       // split-K workspace the launch can use (0: none)
    bool reduce_kpar;        // ... reduced by splitk_reduce_kpar_kernel: never (the plain reduce keeps this route's summation order)
};

// Plan conv_gather_kernel for one op (its classes share one launch): pure, geometry in, plan out.
int plan_gather(const ConvOp &op, GatherPlan &pl) {
    const ClassSpec *cls = op.cls;
    const int ncls = op.ncls, Tmax = op.Tmax, TAmax = op.TAmax, TBmax = op.TBmax, OHc = op.OHc, OWc = op.OWc;
    if (ncls < 1 || ncls > 4) return DVF_ERR_INVALID_ARG;
    GatherArgs &a = pl.a;
    a = GatherArgs{};
    for (int s = 0; s < op.nseg; ++s) a.segC[s] = op.segC[s];
    a.nseg = op.nseg; a.w_mode = op.w_mode;
    a.Mtot = op.Mtot; a.Rtot = op.Rtot; a.KK = op.KK; a.m_base = op.m_base; a.M = op.M;
    a.N = op.N; a.IH = op.IH; a.IW = op.IW; a.OH = op.OH; a.OW = op.OW;
    a.act = op.act; a.alpha = op.alpha; a.beta = op.beta;
    a.ncls = ncls; a.OS = cls[0].OS; a.IS = cls[0].IS;
    for (int i = 0, tap0 = 0; i < ncls; ++i) {
        const ClassSpec &c = cls[i];
        const int T = c.TA * c.TB;
        if (tap0 + T > 52) return DVF_ERR_INVALID_ARG;
        a.cls[i] = ClassDev{c.py, c.px, c.by, c.bx, c.TA, c.TB, c.OHc, c.OWc, tap0};
        for (int t = 0; t < T; ++t) a.tapmap[tap0 + t] = c.tapmap[t];
        tap0 += T;
    }
    // Tile choice: measured on MI355X, large block tiles + split-K beat small tiles without it (the per-chunk
    // staging cost is per block, so 4x smaller tiles stage 4x more per MFMA).
    const int maxBW = ((64 - 1) * cls[0].IS + TBmax > 128) ? 32 : 64;
    const int MT = a.M > 32 ? 2 : 1;
    int NT = 2;
    TilePlan tp = plan_tiles(OHc, OWc, NT, maxBW);
    int64_t nblk = (int64_t)cdiv(OWc, tp.TGX << tp.lsw) * cdiv(OHc, tp.TGY << tp.lsh) * cdiv(a.M, 32 * MT) * a.N * ncls;
    if (nblk < 768) {
        NT = 1;
        tp = plan_tiles(OHc, OWc, NT, maxBW);
        nblk = (int64_t)cdiv(OWc, tp.TGX << tp.lsw) * cdiv(OHc, tp.TGY << tp.lsh) * cdiv(a.M, 32 * MT) * a.N * ncls;
    }
    const int mtiles = cdiv(a.M, 32 * MT);
    a.lsw = tp.lsw; a.lsh = tp.lsh; a.TGX = tp.TGX;
    a.BW = tp.TGX << tp.lsw; a.BH = tp.TGY << tp.lsh;
    if ((a.BW - 1) * a.IS + TBmax > 128) return DVF_ERR_UNSUPPORTED;   // patch rows are staged in <= 2 passes of 64
    a.tilesX = cdiv(OWc, a.BW);
    a.tilesY = cdiv(OHc, a.BH);
    const int PH = (a.BH - 1) * a.IS + TAmax, PW = (a.BW - 1) * a.IS + TBmax, PWH = (PW + 1) / 2;
    a.PSmax = PH * ((a.IS == 2) ? 2 * PWH : PW);
    a.Tmax = Tmax;
    const int COTP = 32 * MT + 1;
    int maxc = 0;
    for (int s = 0; s < a.nseg; ++s) maxc = a.segC[s] > maxc ? a.segC[s] : maxc;
    // largest chunk (2,4,8,16 channels) whose LDS footprint stays <= 40 KiB (3+ blocks per CU)
    auto lds_bytes = [&](int CK) {
        const int WD = (a.w_mode == 0 ? CK : 32 * MT) * a.KK;
        return ((size_t)CK * a.PSmax + (size_t)Tmax * CK * COTP + WD + Tmax + 64) * 4;
    };
    int CK = 16;
    static const size_t g_lds_cap = (dvf_tune("DVF_G_LDS_KB") ? atoi(dvf_tune("DVF_G_LDS_KB")) : 40) * 1024;     // tuning knob
    while (CK > 2 && lds_bytes(CK) > g_lds_cap) CK >>= 1;
    while (CK > 2 && CK / 2 >= maxc) CK >>= 1;
    if (lds_bytes(CK) > 64 * 1024) return DVF_ERR_UNSUPPORTED;
    a.WD = (a.w_mode == 0 ? CK : 32 * MT) * a.KK;
    a.NCH = 0;
    for (int s = 0; s < a.nseg; ++s) a.NCH += cdiv(a.segC[s], CK);
    int KS = 1;
    if (nblk < 384) KS = (int)((512 + nblk - 1) / nblk);
    if (KS > a.NCH) KS = a.NCH;
    if (KS < 1) KS = 1;
    if ((int64_t)a.N * KS * ncls > 65535) return DVF_ERR_UNSUPPORTED;
    a.KS = KS;
    // the kernels address each tensor with 32-bit byte offsets
    for (int s2 = 0; s2 < a.nseg; ++s2)
        if ((int64_t)a.N * a.segC[s2] * a.IH * a.IW * 4 >= ((int64_t)1 << 31) - 16) return DVF_ERR_UNSUPPORTED;
    if ((int64_t)a.Mtot * a.Rtot * a.KK * 4 >= ((int64_t)1 << 31) - 16) return DVF_ERR_UNSUPPORTED;
    pl.MT = MT; pl.NT = NT; pl.CKH = CK / 2; pl.lds = lds_bytes(CK);
    pl.grid = dim3(a.tilesX * a.tilesY, mtiles, a.N * KS * ncls);
    pl.ws_floats = (op.covers && KS > 1) ? (int64_t)KS * a.N * a.M * a.OH * a.OW : 0;
    pl.reduce_kpar = false;
    return DVF_OK;
}

template <int MT, int NT>
int launch_gather_ck(const GatherArgs &a, const GatherPlan &pl, hipStream_t st) {
    switch (pl.CKH) {
        case 1: conv_gather_kernel<MT, NT, 1><<<pl.grid, 256, pl.lds, st>>>(a); break;
        case 2: conv_gather_kernel<MT, NT, 2><<<pl.grid, 256, pl.lds, st>>>(a); break;
        case 4: conv_gather_kernel<MT, NT, 4><<<pl.grid, 256, pl.lds, st>>>(a); break;
        case 8: conv_gather_kernel<MT, NT, 8><<<pl.grid, 256, pl.lds, st>>>(a); break;
        default: return DVF_ERR_UNSUPPORTED;
    }
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

// Launch a planned op: output mode and finish as on the pipelined route (conv_pipe_host.h), with the plain ordered reduce.
int run_gather(const ConvOp &op, const GatherPlan &pl, const ConvIO &io, const float *w, float *ws, int64_t ws_floats,
               hipStream_t st) {
    GatherArgs a = pl.a;
    for (int s = 0; s < a.nseg; ++s) a.in[s] = io.in[s];
    a.w = w; a.bias = io.bias; a.mask = io.mask;
    int rc = prepare_output(a, out_mode_of(op.covers, a.KS, ws, ws_floats, pl.ws_floats), io.out, ws, st);
    if (rc) return rc;
    if (const char *e = dvf_tune("DVF_DBG")) a.dbg = atoi(e);     // ablation switches for tools/conv_bench.py only
    if (pl.MT == 2 && pl.NT == 2) rc = launch_gather_ck<2, 2>(a, pl, st);
    else if (pl.MT == 2) rc = launch_gather_ck<2, 1>(a, pl, st);
    else if (pl.NT == 2) rc = launch_gather_ck<1, 2>(a, pl, st);
    else rc = launch_gather_ck<1, 1>(a, pl, st);
    if (rc) return rc;
    dvf_note_gather(pl.MT, pl.NT, 2 * pl.CKH, a.KS, (int)pl.lds, a.out_mode, a.ncls);
    return finish_output(a, pl.reduce_kpar, ws, io.out, st);
}

// ------------------------------------------------------------------------------------- forward / dgrad routing
// The direct forward kernel of this layer, if one takes it on the unpacked route (the wide heads normally arrive packed).
enum FwdDirect { FWD_NONE, FWD_HEAD, FWD_HEAD_WIDE, FWD_DCONVT };
FwdDirect fwd_direct(const dvf_conv_desc *d, int nseg) {
    if (dvf_head_applicable(d, nseg)) return FWD_HEAD;
    if (dvf_head_wide_applicable(d, nseg)) return FWD_HEAD_WIDE;
    if (dvf_dconvt_applicable(d, nseg)) return FWD_DCONVT;            // thin stride-2 transposed convolutions
    return FWD_NONE;
}

// Forward through the unpacked kernels: a direct kernel, else conv_gather_kernel.
int fwd_unpacked(const dvf_conv_desc *d, const ConvOp &op, const ConvIO &io, const int *seg_channels, int nseg, const float *w,
                 float *ws, int64_t ws_floats, hipStream_t st) {
    switch (fwd_direct(d, nseg)) {
        case FWD_HEAD: return dvf_head_fwd(d, io.in[0], w, io.bias, io.out, st);
        case FWD_HEAD_WIDE: return dvf_head_fwd_segs(d, io.in, seg_channels, nseg, w, io.bias, io.out, st);
        case FWD_DCONVT: return dvf_dconvt_fwd(d, io.in[0], w, io.bias, io.out, st);
        case FWD_NONE: break;
    }
    GatherPlan pl;
    const int rc = plan_gather(op, pl);
    return rc ? rc : run_gather(op, pl, io, w, ws, ws_floats, st);
}

// dgrad of one input segment with the unpacked weights: the head kernel for narrow segments, else conv_gather_kernel.
int dgrad_unpacked(const dvf_conv_desc *d, const ConvOp &op, const ConvIO &io, const float *w, float *ws, int64_t ws_floats,
                   hipStream_t st) {
    if (dvf_head_seg_dgrad_applicable(d, op.M))
        return dvf_head_seg_dgrad(d, io.in[0], w, io.out, op.m_base, op.M, st, io.mask);     // (mask applied in the kernel)
    GatherPlan pl;
    const int rc = plan_gather(op, pl);
    return rc ? rc : run_gather(op, pl, io, w, ws, ws_floats, st);     // (mask applied in the kernel or its finish)
}

// Split-K workspace the unpacked route of an op can use.
int64_t unpacked_ws_floats(const ConvOp &op, bool direct) {
    if (direct) return 0;
    GatherPlan pl;
    const int rc = plan_gather(op, pl);
    return rc ? rc : pl.ws_floats;
}

// One input segment of a dgrad: its op and, when it runs pipelined, its plan and where its share of the packed buffer begins.
struct DgradSeg {
    int s, off;              // segment index, first channel
    ConvOp op;
    bool packed;             // plan is valid; false: the unpacked kernels take the segment
    PipePlan plan;
    int64_t packed_off;      // floats
};

// The one walk over the segments of a dgrad.  use_pipe false: unpacked kernels only (nothing is planned).
template <class F>
int for_each_dgrad_seg(const dvf_conv_desc *d, const int *seg_channels, int nseg, bool use_pipe, F visit) {
    DgradSeg v;
    v.off = 0; v.packed_off = 0;
    for (v.s = 0; v.s < nseg; ++v.s) {
        int rc = make_dgrad_op(d, v.off, seg_channels[v.s], v.op);
        v.packed = false;
        if (use_pipe) {
            if (rc) return rc;
            rc = plan_pipe(v.op, v.plan);
            if (rc && rc != DVF_ERR_UNSUPPORTED) return rc;
            v.packed = !rc;
        }
        rc = visit(v);
        if (rc) return rc;
        if (v.packed) v.packed_off += v.plan.packed_floats;    // (an unpacked segment has no packed share)
        v.off += seg_channels[v.s];
    }
    return DVF_OK;
}

int64_t conv_sizes(const dvf_conv_desc *d, const int *seg_channels, int nseg, int op_kind, bool want_ws) {
    int rc = check_desc(d);
    if (rc) return rc;
    rc = check_segs(d, seg_channels, nseg);
    if (rc) return rc;
    if (op_kind == 0) {
        if (!want_ws && dvf_dconvt_applicable(d, nseg)) return DVF_ERR_UNSUPPORTED;   // (forward runs the direct kernel)
        ConvOp op;
        PipePlan pl;
        rc = make_fwd_op(d, seg_channels, nseg, op);
        if (rc) return rc;
        rc = plan_pipe(op, pl);
        if (rc == DVF_ERR_UNSUPPORTED && want_ws) return unpacked_ws_floats(op, fwd_direct(d, nseg) != FWD_NONE);
        return rc ? rc : (want_ws ? pl.ws_floats : pl.packed_floats);
    }
    if (op_kind != 1) return DVF_ERR_INVALID_ARG;
    int64_t total = 0, wmax = 0;
    int nsup = 0;
    rc = for_each_dgrad_seg(d, seg_channels, nseg, true, [&](const DgradSeg &v) -> int {
        int64_t wf = 0;
        if (v.packed) {
            total += v.plan.packed_floats;
            wf = v.plan.ws_floats;
            ++nsup;
        } else if (want_ws) {
            wf = unpacked_ws_floats(v.op, dvf_head_seg_dgrad_applicable(d, v.op.M));
            if (wf < 0) return (int)wf;
        }
        wmax = wf > wmax ? wf : wmax;
        return DVF_OK;
    });
    if (rc) return rc;
    if (!nsup && !want_ws) return DVF_ERR_UNSUPPORTED;
    return want_ws ? wmax : total;
}

// ------------------------------------------------------------------------------------- weight gradient
// Roles of the weight gradient of input segment s (s < 0, Conv2d only: of the virtual concatenation of all segments):
//   Conv2d           dW[co][ci][a][b] = sum dpre[co][o] * in[ci][o*s - p + (a,b)]       P = dpre, Q = input
//   ConvTranspose2d  dW[ci][co][a][b] = sum in[ci][i] * dpre[co][i*s - p + (a,b)]       P = input segment, Q = dpre
WgradArgs wgrad_args(const dvf_conv_desc *d, const float *const *in_segs, const int *seg_channels, int s, const float *dpre,
                     float *dw) {
    int off = 0;
    for (int i = 0; i < s; ++i) off += seg_channels[i];
    const int segc = s < 0 ? d->C_in : seg_channels[s];
    WgradArgs a{};
    a.KK = d->KH * d->KW; a.KH = d->KH; a.KW = d->KW; a.N = d->N; a.S = d->stride; a.pad = d->pad; a.G = dw;
    if (!d->transposed) {
        a.P = dpre; a.PCtot = d->C_out; a.m_base = 0; a.M = d->C_out; a.GH = d->H_out; a.GW = d->W_out;
        a.Q = s < 0 ? nullptr : in_segs[s]; a.QCtot = segc; a.q_base = 0; a.Cq = segc; a.QH = d->H_in; a.QW = d->W_in;
        a.g_mstride = (int64_t)d->C_in * a.KK; a.g_mbase = 0; a.g_cbase = off;
    } else {
        a.P = in_segs[s]; a.PCtot = segc; a.m_base = 0; a.M = segc; a.GH = d->H_in; a.GW = d->W_in;
        a.Q = dpre; a.QCtot = d->C_out; a.q_base = 0; a.Cq = d->C_out; a.QH = d->H_out; a.QW = d->W_out;
        a.g_mstride = (int64_t)d->C_out * a.KK; a.g_mbase = off; a.g_cbase = 0;
    }
    return a;
}

struct WgradPipePlan {
    WgpArgs w;               // geometry and tiling; the operands are set at launch
    int MT, NTW, TILE, nblocks;
    size_t lds;
    int64_t ws_floats;       // scratch of the deterministic flush (wgrad_pipe.h)
};

// Plan the pipelined weight-gradient kernel (wgrad_pipe.hip) for the roles in `o` with Q = the virtual concatenation of nseg
// tensors of qsegc[s] channels: pure.  aligned16: P and every Q segment are 16-byte aligned; want_bias (Conv2d roles): the
// launch should also sum P per channel if it has a spare column.  DVF_ERR_UNSUPPORTED when the geometry is outside the
// kernel's envelope (the register-staged conv_wgrad_kernel then takes it).
int plan_wgrad_pipe(const WgradArgs &o, const int *qsegc, int nseg, bool aligned16, bool want_bias, WgradPipePlan &pl) {
    static const bool off = dvf_tune("DVF_WG_PIPE") && atoi(dvf_tune("DVF_WG_PIPE")) == 0;     // tuning knob
    if (off) return DVF_ERR_UNSUPPORTED;
    const int T = o.KH * o.KW;
    if ((o.S != 1 && o.S != 2) || T > 128 || o.pad < 0 || o.pad > 4) return DVF_ERR_UNSUPPORTED;
    if ((int64_t)o.N * o.PCtot * o.GH * o.GW * 4 >= ((int64_t)1 << 31) - 16 ||
        nseg < 1 || nseg > DVF_MAX_SEGS)
        return DVF_ERR_UNSUPPORTED;                 // 32-bit byte offsets inside the kernel
    WgpArgs &w = pl.w;
    w = WgpArgs{};
    for (int s = 0; s < nseg; ++s) {
        if ((int64_t)o.N * qsegc[s] * o.QH * o.QW * 4 >= ((int64_t)1 << 31) - 16) return DVF_ERR_UNSUPPORTED;
        w.segC[s] = qsegc[s];
    }
    w.nseg = nseg;
    w.PCtot = o.PCtot; w.m_base = o.m_base; w.M = o.M; w.Cq = o.Cq;
    w.g_mstride = o.g_mstride; w.g_mbase = o.g_mbase; w.g_cbase = o.g_cbase; w.KK = o.KK; w.KH = o.KH; w.KW = o.KW;
    w.N = o.N; w.GH = o.GH; w.GW = o.GW; w.QH = o.QH; w.QW = o.QW; w.S = o.S; w.pad = o.pad;
    w.XA = (o.pad + 3) & ~3;
    w.RSq = roundup(w.XA + (WGP_BW - 1) * o.S + o.KW - o.pad, 4);
    w.PHq = (WGP_BH - 1) * o.S + o.KH;
    w.x4 = (o.GW % 4 == 0 && o.QW % 4 == 0 && aligned16) ? 1 : 0;
    if (const char *e = dvf_tune("DVF_WG_X4")) w.x4 = w.x4 && atoi(e) != 0;      // tuning knob: 0 = 4-byte DMA lanes everywhere
    const int piece = w.x4 ? 256 : 64;
    w.NPIq = cdiv(w.PHq * w.RSq, piece);
    if (w.NPIq > WGP_MAXQ) return DVF_ERR_UNSUPPORTED;
    w.PSq = w.NPIq * piece + 4;
    // Block shape: TILE*MT rows x 4*NTW*TILE columns, MFMA 32x32x2 (TILE 32) or 16x16x4 (TILE 16: same rate, a quarter of
    // the tile).  Cost ~ matrix-pipe cycles of the layer = m-blocks x channel chunks x MT x NTW x (4 | 1); the 16-wide tiles
    // only when they save >= 15 % (small row / column counts: a 32-wide tile would be mostly padding) -- per MFMA they read
    // more LDS and re-stage more of P.  Channel chunks are balanced.
    static const bool no16 = dvf_tune("DVF_WG_TILE16") && atoi(dvf_tune("DVF_WG_TILE16")) == 0;      // tuning knob
    double best_cost = 1e30;
    int TILE = 0, MT = 0, NTW = 0, CK = 0;
    for (int tile = 32; tile >= 16; tile -= 16) {
        if (tile == 16 && no16) break;
        for (int mt = 2; mt >= 1; --mt) {
            if (mt == 2 && o.M <= tile) continue;                 // (a second row tile would be empty)
            const int pf = (tile * mt / 2) * WGP_PAIR;
            for (int ntw = (tile == 16 ? 4 : 2); ntw >= 1; --ntw) {
                int ckmax = (4 * ntw * tile) / T;
                if (ckmax > o.Cq) ckmax = o.Cq;
                while (ckmax >= 1 && (size_t)2 * (pf + (size_t)(ckmax + 1) * w.PSq) * 4 > WGP_LDS_CAP) --ckmax;   // (+1: slot of ones)
                if (ckmax < 1) continue;
                const int nch = cdiv(o.Cq, ckmax);
                double cost = (double)cdiv(o.M, tile * mt) * nch * mt * ntw * (tile == 32 ? 4 : 1);
                if (tile == 16) cost *= 1.15;
                if (cost < best_cost) { best_cost = cost; TILE = tile; MT = mt; NTW = ntw; CK = cdiv(o.Cq, nch); }
            }
        }
    }
    const int MB = TILE * MT, PF = (MB / 2) * WGP_PAIR;
    if (!NTW) return DVF_ERR_UNSUPPORTED;
    w.CK = CK;
    w.mtiles = cdiv(o.M, MB);
    w.cchunks = cdiv(o.Cq, CK);
    w.tilesX = cdiv(o.GW, WGP_BW);
    w.tilesY = cdiv(o.GH, WGP_BH);
    w.ntiles = o.N * w.tilesX * w.tilesY;
    const int64_t W = (int64_t)w.mtiles * w.cchunks * w.ntiles;
    if (W >= ((int64_t)1 << 30)) return DVF_ERR_UNSUPPORTED;
    w.W = (int)W;
    static const int ncu = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
        return n;
    }();
    const int nblocks = w.W < ncu ? w.W : ncu;
    w.bias_col = (want_bias && CK * T < 4 * NTW * TILE) ? CK * T : -1; // a spare column of the tile multiplies by ones
    w.QSLOTS = CK + (w.bias_col >= 0 ? 1 : 0);
    const size_t lds = (size_t)2 * (PF + (size_t)w.QSLOTS * w.PSq) * 4;
    const int64_t need = wgrad_pipe_slots(w, nblocks) * wgrad_pipe_slot_floats(MT, NTW, TILE);
    pl.MT = MT; pl.NTW = NTW; pl.TILE = TILE; pl.nblocks = nblocks; pl.lds = lds; pl.ws_floats = need;
    return DVF_OK;
}

// Launch a planned wgrad_pipe op: G += P x Q (and dbias += sums of P when the plan has the spare column: *bias_done).
int run_wgrad_pipe(const WgradPipePlan &pl, const float *P, const float *const *qsegs, float *G, float *dbias, bool *bias_done,
                   float *ws, int64_t ws_floats, hipStream_t st) {
    WgpArgs w = pl.w;
    w.P = P; w.G = G;
    for (int s = 0; s < w.nseg; ++s) w.Q[s] = qsegs[s];
    w.dbias = w.bias_col >= 0 ? dbias : nullptr;
    w.ws = (ws && ws_floats >= pl.ws_floats) ? ws : nullptr;
    if (const char *e = dvf_tune("DVF_WG_DBG")) w.dbg = atoi(e);
    w.stamps = nullptr;
#ifdef DVF_TUNING
    if (dvf_tune("DVF_WG_STAMPS")) {   // in-kernel cycle account of the LAST wgrad_pipe launch (tools/r3/stamps.py)
        if (!g_stamp_buf && hipMalloc(&g_stamp_buf, STAMP_MAX_BLOCKS * 64) != hipSuccess) return DVF_ERR_LAUNCH;
        if ((size_t)pl.nblocks <= STAMP_MAX_BLOCKS) {
            if (hipMemsetAsync(g_stamp_buf, 0, (size_t)pl.nblocks * 64, st) != hipSuccess) return DVF_ERR_LAUNCH;
            w.stamps = g_stamp_buf;
            g_stamp_blocks = pl.nblocks;
        }
    }
#endif
    int rc = dvf_wgrad_pipe_launch(w, pl.MT, pl.NTW, pl.nblocks, pl.lds, st, pl.TILE);
    if (rc == DVF_OK && w.ws) rc = dvf_wgrad_pipe_reduce(w, pl.MT, pl.NTW, pl.nblocks, st, pl.TILE);
    if (rc) return rc;
    dvf_note_wgrad_pipe(pl.MT, pl.TILE, pl.NTW, w.x4, w.ws != nullptr, w.CK, w.S, w.NPIq, pl.nblocks, (int)pl.lds, w.KH * w.KW, w.RSq,
                        w.nseg);
    if (bias_done) *bias_done = w.bias_col >= 0;
    return DVF_OK;
}

bool aligned16(const float *p, const float *const *q, int n) {
    uintptr_t v = reinterpret_cast<uintptr_t>(p);
    for (int s = 0; s < n; ++s) v |= reinterpret_cast<uintptr_t>(q[s]);
    return (v & 15) == 0;
}

// Weight gradient, top to bottom: the direct head kernel; wgrad_pipe over the virtual concatenation (Conv2d) or per input
// segment (transposed); the register-staged conv_wgrad_kernel, per segment, for what wgrad_pipe refuses.
// *bias_done: the launch also added the channel sums of dpre to dbias.
int wgrad_route(const dvf_conv_desc *d, const float *const *in_segs, const int *seg_channels, int nseg, const float *dpre,
                float *dw, int accumulate, float *dbias, bool *bias_done, float *ws, int64_t ws_floats, hipStream_t st) {
    *bias_done = false;
    if (dvf_head_applicable(d, nseg)) {
        if (!in_segs[0]) return DVF_ERR_INVALID_ARG;
        return dvf_head_wgrad(d, in_segs[0], dpre, dw, accumulate, st, ws, ws_floats);
    }
    if (!accumulate && hipMemsetAsync(dw, 0, sizeof(float) * (size_t)d->C_in * d->C_out * d->KH * d->KW, st) != hipSuccess)
        return DVF_ERR_LAUNCH;
    for (int s = 0; s < nseg; ++s)
        if (!in_segs[s]) return DVF_ERR_INVALID_ARG;
    WgradPipePlan pp;
    if (!d->transposed) {
        const WgradArgs a = wgrad_args(d, in_segs, seg_channels, -1, dpre, dw);
        int rc = plan_wgrad_pipe(a, seg_channels, nseg, aligned16(dpre, in_segs, nseg), dbias != nullptr, pp);
        if (!rc) rc = run_wgrad_pipe(pp, dpre, in_segs, dw, dbias, bias_done, ws, ws_floats, st);
        if (rc != DVF_ERR_UNSUPPORTED) return rc;
    }
    for (int s = 0; s < nseg; ++s) {
        WgradArgs a = wgrad_args(d, in_segs, seg_channels, s, dpre, dw);
        int rc = DVF_ERR_UNSUPPORTED;
        if (d->transposed) {
            rc = plan_wgrad_pipe(a, &d->C_out, 1, aligned16(a.P, &dpre, 1), false, pp);
            if (!rc) rc = run_wgrad_pipe(pp, a.P, &dpre, dw, nullptr, nullptr, ws, ws_floats, st);
        }
        if (rc == DVF_ERR_UNSUPPORTED) {
            WgradRegPlan rp;
            rc = plan_wgrad_reg(a, rp);
            if (!rc) rc = launch_wgrad_reg(a, rp, st);
        }
        if (rc) return rc;
    }
    return DVF_OK;
}

}  // namespace

extern "C" {

int64_t dvf_conv2d_wgrad_ws_floats(const dvf_conv_desc *d, const int *seg_channels, int nseg) {
    int rc = check_desc(d);
    if (rc) return rc;
    rc = check_segs(d, seg_channels, nseg);
    if (rc) return rc;
    int64_t need = 0;
    if (dvf_head_applicable(d, nseg)) {
        need = dvf_head_wgrad_ws_floats(d);
    } else {
        // planned for 16-byte aligned operands; transposed layers launch once per input segment and reuse the scratch, so
        // the largest launch counts
        const float *const none[DVF_MAX_SEGS] = {};
        WgradPipePlan pp;
        auto plan = [&](int s, const int *qsegc, int qnseg) {
            const WgradArgs a = wgrad_args(d, none, seg_channels, s, nullptr, nullptr);
            if (plan_wgrad_pipe(a, qsegc, qnseg, true, false, pp) == DVF_OK && pp.ws_floats > need) need = pp.ws_floats;
        };
        if (!d->transposed) plan(-1, seg_channels, nseg);
        else for (int s = 0; s < nseg; ++s) plan(s, &d->C_out, 1);
    }
    const int64_t nb = dvf_act_bwd_ws_floats(d->N, d->C_out, d->H_out * d->W_out);      // (the bias pass behind it, when one runs)
    return need > nb ? need : nb;
}

int dvf_conv2d_wgrad(const dvf_conv_desc *d, const float *const *in_segs, const int *seg_channels, int nseg,
                     const float *dpre, float *dw, int accumulate, float *dbias, int accumulate_dbias, float *ws,
                     int64_t ws_floats, void *stream) {
    if (!d) return DVF_ERR_INVALID_ARG;
    hipStream_t st = dvf_stream(stream);
    if (dbias && !accumulate_dbias &&
        hipMemsetAsync(dbias, 0, sizeof(float) * (size_t)(d->C_out > 0 ? d->C_out : 0), st) != hipSuccess)
        return DVF_ERR_LAUNCH;
    dvf_plan_reset();
    int rc = check_desc(d);
    if (rc) return rc;
    rc = check_segs(d, seg_channels, nseg);
    if (rc) return rc;
    if (!in_segs || !dpre || !dw) return DVF_ERR_INVALID_ARG;
    bool done = false;
    rc = wgrad_route(d, in_segs, seg_channels, nseg, dpre, dw, accumulate, dbias, &done, ws, ws_floats, st);
    if (rc || done || !dbias) return rc;
    // the weight-gradient launch had no spare column (or ran another kernel): one pass over dpre
    return dvf_act_bwd(dpre, nullptr, nullptr, dbias, d->N, d->C_out, d->H_out * d->W_out, DVF_ACT_NONE, 1.f, 0.f, 1, ws, ws_floats, stream);
}

static int act_bwd_chunks(int N, int C, int HW, bool has_bias) {
    int chunks = (HW + 8191) / 8192;
    const int64_t planes = (int64_t)N * C;
    while (chunks > 1 && planes * chunks > 16384) chunks >>= 1;
    // small layers: still fill the GPU -- but every block ends in ONE float atomic on dbias[c], and atomics on one address
    // serialise (~40 ns each: 1024 blocks of a 1-channel head cost 41 us for a 10 MB pass): at most ~128 blocks per channel
    while (planes * chunks < 1024 && HW / (chunks * 2) >= 1024 && (!has_bias || (int64_t)N * chunks * 2 <= 128)) chunks *= 2;
    return chunks;
}

// Blocks per plane of bias_sum_kernel: planes are split only while the grid is short of one block per CU and a block keeps
// at least 32 KB; the atomics on one 64-byte line of dbias (16 channels) then number a few hundred at most.
static int bias_sum_chunks(int N, int C, int HW) {
    int target = 256;
    if (const char *t = dvf_tune("DVF_BIAS_BLOCKS")) target = atoi(t);
    int chunks = 1;
    while ((int64_t)N * C * chunks * 2 <= target && HW / (chunks * 2) >= 8192) chunks *= 2;
    return chunks;
}

int64_t dvf_act_bwd_ws_floats(int N, int C, int HW) {
    if (N <= 0 || C <= 0 || HW <= 0) return DVF_ERR_INVALID_ARG;
    const int a = act_bwd_chunks(N, C, HW, true), b = bias_sum_chunks(N, C, HW);      // (either pass may run)
    return (int64_t)C * N * (a > b ? a : b);
}

int dvf_act_bwd(const float *dy, const float *y, float *dpre, float *dbias, int N, int C, int HW, int act, float alpha,
                float beta, int accumulate_dbias, float *ws, int64_t ws_floats, void *stream) {
    if (!dy || (act != DVF_ACT_NONE && !y) || N <= 0 || C <= 0 || HW <= 0) return DVF_ERR_INVALID_ARG;
    if (!dpre && !dbias) return DVF_OK;
    hipStream_t st = dvf_stream(stream);
    if (dbias && !accumulate_dbias && hipMemsetAsync(dbias, 0, sizeof(float) * C, st) != hipSuccess) return DVF_ERR_LAUNCH;
    const bool vec = (HW % 4 == 0) && ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(y) |
                                        reinterpret_cast<uintptr_t>(dpre)) % 16 == 0);
    const bool sums_only = !dpre && act == DVF_ACT_NONE;
    const int chunks = sums_only ? bias_sum_chunks(N, C, HW) : act_bwd_chunks(N, C, HW, dbias != nullptr);
    const int64_t planes = (int64_t)N * C;
    // with the scratch: per-block partial sums, added in index order by bias_finish_kernel (else float atomics on dbias)
    float *part = (dbias && ws && ws_floats >= dvf_act_bwd_ws_floats(N, C, HW)) ? ws : nullptr;
    if (sums_only) {
        const int per = ((vec ? HW >> 2 : HW) + chunks - 1) / chunks;          // loads per block
        const int threads = per <= 256 ? 64 : per <= 8192 ? 256 : 1024;
        if (vec) bias_sum_kernel<true><<<(unsigned)(planes * chunks), threads, 0, st>>>(dy, dbias, C, HW, chunks, part, N * chunks);
        else bias_sum_kernel<false><<<(unsigned)(planes * chunks), threads, 0, st>>>(dy, dbias, C, HW, chunks, part, N * chunks);
    } else if (vec) act_bwd_kernel<true><<<(unsigned)(planes * chunks), 256, 0, st>>>(dy, y, dpre, dbias, C, HW, act, alpha, beta, chunks, part, N * chunks);
    else act_bwd_kernel<false><<<(unsigned)(planes * chunks), 256, 0, st>>>(dy, y, dpre, dbias, C, HW, act, alpha, beta, chunks, part, N * chunks);
    DVF_LAUNCH_CHECK();
    if (part) {
        bias_finish_kernel<<<C, 64, 0, st>>>(part, dbias, N * chunks);
        DVF_LAUNCH_CHECK();
    }
    return DVF_OK;
}


// ---- packed-weight fast path (conv_pipe_kernel)
int64_t dvf_conv2d_packed_floats(const dvf_conv_desc *d, const int *seg_channels, int nseg, int op_kind) {
    return conv_sizes(d, seg_channels, nseg, op_kind, false);
}

int64_t dvf_conv2d_ws_floats(const dvf_conv_desc *d, const int *seg_channels, int nseg, int op_kind) {
    return conv_sizes(d, seg_channels, nseg, op_kind, true);
}

int dvf_conv2d_pack(const dvf_conv_desc *d, const int *seg_channels, int nseg, int op_kind, const float *w, float *packed,
                    void *stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    rc = check_segs(d, seg_channels, nseg);
    if (rc) return rc;
    if (!w || !packed) return DVF_ERR_INVALID_ARG;
    hipStream_t st = dvf_stream(stream);
    if (op_kind == 0) {
        ConvOp op;
        PipePlan pl;
        rc = make_fwd_op(d, seg_channels, nseg, op);
        if (!rc) rc = plan_pipe(op, pl);
        return rc ? rc : launch_pack(op, pl, w, packed, st);
    }
    if (op_kind != 1) return DVF_ERR_INVALID_ARG;
    return for_each_dgrad_seg(d, seg_channels, nseg, true, [&](const DgradSeg &v) -> int {
        return v.packed ? launch_pack(v.op, v.plan, w, packed + v.packed_off, st) : DVF_OK;
    });
}

int dvf_conv2d_fwd(const dvf_conv_desc *d, const float *const *in_segs, const int *seg_channels, int nseg,
                   const float *packed, const float *w, const float *bias, float *out, float *ws, int64_t ws_floats,
                   void *stream) {
    dvf_plan_reset();
    int rc = check_desc(d);
    if (rc) return rc;
    rc = check_segs(d, seg_channels, nseg);
    if (rc) return rc;
    if (!in_segs || !w || !out) return DVF_ERR_INVALID_ARG;
    for (int s = 0; s < nseg; ++s)
        if (!in_segs[s]) return DVF_ERR_INVALID_ARG;
    hipStream_t st = dvf_stream(stream);
    const ConvIO io{in_segs, bias, out, nullptr};
    ConvOp op;
    rc = make_fwd_op(d, seg_channels, nseg, op);     // (DVF_ERR_UNSUPPORTED: no class has a tap -- nothing to run pipelined)
    if (packed && !rc) {
        PipePlan pl;
        rc = plan_pipe(op, pl);
        if (!rc) rc = run_pipe(op, pl, io, packed, ws, ws_floats, st);
        // refused for this geometry, or at run time (an operand of a 16-byte-lane plan is not 16-byte aligned): the
        // unpacked kernels take the call -- run_pipe refuses before it notes a plan or launches anything
        if (rc != DVF_ERR_UNSUPPORTED) return rc;
    }
    return fwd_unpacked(d, op, io, seg_channels, nseg, w, ws, ws_floats, st);
}

// dgrad of every requested segment; packed == NULL: unpacked kernels only.  mask_segs[s] != NULL: segment s was produced
// by a ReLU layer whose output is mask_segs[s]; its gradient leaves already multiplied by relu'() (in the kernel's
// epilogue / its split-K finish, or a pass of act_bwd_kernel after it).
int dvf_conv2d_dgrad(const dvf_conv_desc *d, const float *dpre, const float *packed, const float *w, float *const *din_segs,
                     const int *seg_channels, int nseg, float *ws, int64_t ws_floats, const float *const *mask_segs,
                     void *stream) {
    dvf_plan_reset();
    int rc = check_desc(d);
    if (rc) return rc;
    rc = check_segs(d, seg_channels, nseg);
    if (rc) return rc;
    if (!dpre || !w || !din_segs) return DVF_ERR_INVALID_ARG;
    hipStream_t st = dvf_stream(stream);
    auto mask = [&](int s) -> const float * { return mask_segs ? mask_segs[s] : nullptr; };
    if (dvf_head_dgrad_applicable(d, nseg) || (dvf_head_applicable(d, nseg) && !packed))
        return din_segs[0] ? dvf_head_dgrad(d, dpre, w, din_segs[0], st, mask(0)) : DVF_OK;     // (mask applied in the kernel)
    return for_each_dgrad_seg(d, seg_channels, nseg, packed != nullptr, [&](const DgradSeg &v) -> int {
        if (!din_segs[v.s]) return DVF_OK;
        const ConvIO io{&dpre, nullptr, din_segs[v.s], mask(v.s)};
        int r = v.packed ? run_pipe(v.op, v.plan, io, packed + v.packed_off, ws, ws_floats, st) : DVF_ERR_UNSUPPORTED;
        // a narrow segment, or one refused at run time (an operand of a 16-byte-lane plan is not 16-byte aligned): it runs
        // unpacked, masked or not -- the caller must not have to know which of its segments were packed
        if (r == DVF_ERR_UNSUPPORTED) r = dgrad_unpacked(d, v.op, io, w, ws, ws_floats, st);
        return r;
    });
}

// ---- batched packing: every convolution's job in one launch per optimizer step
int dvf_conv2d_pack_jobs(const dvf_conv_desc *d, const int *seg_channels, int nseg, int op_kind, const float *w, float *packed,
                         void *jobs_host, int max_jobs, int *blocks_out, int *lds_bytes_out) {
    static_assert(sizeof(PackArgs) <= DVF_PACK_JOB_BYTES, "DVF_PACK_JOB_BYTES too small");
    int rc = check_desc(d);
    if (rc) return rc;
    rc = check_segs(d, seg_channels, nseg);
    if (rc) return rc;
    if (!w || !packed || !jobs_host || !blocks_out || max_jobs < 1) return DVF_ERR_INVALID_ARG;
    char *out = static_cast<char *>(jobs_host);
    int njobs = 0;
    auto emit = [&](const ConvOp &op, const PipePlan &pl, float *dst) {
        const PackArgs job = pack_job(op, pl, w, dst, &blocks_out[njobs]);
        memset(out + (size_t)njobs * DVF_PACK_JOB_BYTES, 0, DVF_PACK_JOB_BYTES);
        memcpy(out + (size_t)njobs * DVF_PACK_JOB_BYTES, &job, sizeof(job));
        if (lds_bytes_out && (int)pl.pack_lds > *lds_bytes_out) *lds_bytes_out = (int)pl.pack_lds;
        ++njobs;
    };
    if (op_kind == 0) {
        ConvOp op;
        PipePlan pl;
        rc = make_fwd_op(d, seg_channels, nseg, op);
        if (!rc) rc = plan_pipe(op, pl);
        if (rc) return rc;
        emit(op, pl, packed);
        return njobs;
    }
    if (op_kind != 1) return DVF_ERR_INVALID_ARG;
    rc = for_each_dgrad_seg(d, seg_channels, nseg, true, [&](const DgradSeg &v) -> int {
        if (njobs >= max_jobs) return DVF_ERR_INVALID_ARG;
        if (v.packed) emit(v.op, v.plan, packed + v.packed_off);
        return DVF_OK;
    });
    return rc ? rc : njobs;
}

int dvf_conv2d_pack_batch(const void *jobs_dev, const int *block_prefix_dev, const int *block_job_dev, int njobs,
                          int total_blocks, int lds_bytes, void *stream) {
    if (!jobs_dev || !block_prefix_dev || njobs < 1 || total_blocks < 1 || lds_bytes < 4 || lds_bytes > 64 * 1024)
        return DVF_ERR_INVALID_ARG;
    static_assert(DVF_PACK_JOB_BYTES % alignof(PackArgs) == 0, "job stride");
    static_assert(sizeof(PackArgs) == DVF_PACK_JOB_BYTES, "job stride");
    conv_pack_batch_kernel<<<total_blocks, 256, lds_bytes, dvf_stream(stream)>>>(
        static_cast<const PackArgs *>(jobs_dev), block_prefix_dev, block_job_dev, njobs);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

#ifdef DVF_TUNING
// (tuning build only, not part of include/dvf_hip.h) the cycle account of the last pipelined launch made with DVF_STAMPS
// set: 8 x u64 per block (conv_pipe.h), copied to the host after a device synchronisation.  Returns the block count.
int dvf_tuning_read_stamps(unsigned long long *out, int max_blocks) {
    if (!out || !g_stamp_buf) return 0;
    const int nb = g_stamp_blocks < max_blocks ? g_stamp_blocks : max_blocks;
    if (hipDeviceSynchronize() != hipSuccess) return DVF_ERR_LAUNCH;
    if (hipMemcpy(out, g_stamp_buf, (size_t)nb * 64, hipMemcpyDeviceToHost) != hipSuccess) return DVF_ERR_LAUNCH;
    return nb;
}
#endif

}  // extern "C"
