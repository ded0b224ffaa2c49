// Depth validation metrics against ground truth (loss_functions_sfm.py:80-116 of the reference, plus the rmse / rmse_log /
// counts that the Eigen protocol reports): per image the masked error means and the EXACT lower median of the valid ground
// truth and of the clamped prediction, with no host round trip.  Definition of every column: include/dvf_hip.h.
//
// Median = radix select on the bit patterns.  A valid gt is > gt_lo >= 0 and a clamped prediction is >= clamp_lo > 0, so both
// are positive floats and order as uint32 (a NaN prediction sorts last; its row reports NaN anyway).  Three digit passes of
// 11 / 11 / 10 bits:
//   dm_zero_kernel      zeroes the histograms and the select state in ws
//   dm_hist_kernel<0>   histogram of key >> 21 over the valid pixels
//   dm_hist_kernel<1>   resolves digit 0 (scan of histogram 0), histogram of (key >> 10) & 2047 over the keys that share it
//   dm_hist_kernel<2>   resolves digit 1, histogram of key & 1023 over the keys that share both
//   dm_metrics_kernel   resolves digit 2 = the medians, then the error sums of its chunk -> per-block partials
//   dm_finish_kernel    one block per image adds the partials in a fixed order and writes the output row
// Every block of a pass scans the 2 x 2048 bins of the previous pass itself (8 bins per thread, one block-wide prefix sum);
// block 0 of an image also stores the resolved (prefix, remaining rank) so the NEXT pass starts from it and scans one
// histogram only.  Histograms are built in LDS with integer atomics and the non-empty bins flushed with integer global
// atomics; sums go through per-block partials.  Integer adds commute exactly and no float atomic exists anywhere: two runs
// are bit-identical.
//
// LDS contention: depths of one scene share sign, exponent and top mantissa bits, so digit 0 of a wave's 64 pixels lands in a
// handful of bins and 64 lanes adding to one LDS address serialise.  hist_add aggregates once within the wave: the first
// active lane's digit is broadcast, the lanes that hold the same digit are counted with a ballot and ONE lane adds the count;
// whatever is still active adds 1 by itself.  (DESIGN.md section 4 has the measurement against more rounds, plain per-lane
// adds and per-wave sub-histograms; a -DDVF_TUNING build selects those with DVF_DM_HIST.)
#include "dvf_common.h"

namespace {

constexpr int NT = 256, PPT = 8, PPB = NT * PPT;   // one block owns 2048 consecutive pixels of one image
constexpr int BINS = 2048, HIST_U32 = 3 * 2 * BINS, STATE_U32 = 16, NPART = 10, AGG_ROUNDS = 1;
enum { HIST_DIRECT = 0, HIST_AGG = 1, HIST_SUB = 2, HIST_AGG2 = 3, HIST_AGG8 = 4 };   // 0, 2, 3, 4: tuning build only
// partial columns: five float sums, then five integer counts
enum { P_ABS = 0, P_REL, P_SQREL, P_SQ, P_LOGSQ, P_A1, P_A2, P_A3, P_NVALID, P_NNAN };

struct DmArgs {
    const float *gt, *pred;
    uint32_t *hist, *state;   // [B][3][2][BINS], [B][STATE_U32]: (key_gt, rank_gt, key_pred, rank_pred) after each pass
    float *partials, *out;    // [B][nblk][NPART], [B][12]
    int HW, W, y1, y2, x1, x2, nblk;
    float gt_lo, gt_hi, c_lo, c_hi;
    uint32_t flags;
};

static inline int dm_blocks(int H, int W) { return (int)(((int64_t)H * W + PPB - 1) / PPB); }

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v != v ? v : fminf(fmaxf(v, lo), hi); }

// The PPT pixels of this thread (i0, i0 + NT, ...): every load is issued before anything is used, so a block waits for memory
// once.  g = ground truth, p = clamped prediction, bit k of the result = pixel k is valid.
// (indices are unsigned: the last block's run up to PPB - 1 past HW, which may itself be close to 2^31)
__device__ __forceinline__ uint32_t dm_load(const DmArgs &a, int64_t base, uint32_t i0, float (&g)[PPT], float (&p)[PPT]) {
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const uint32_t i = i0 + k * NT;
        const bool in = i < (uint32_t)a.HW;
        g[k] = in ? a.gt[base + i] : 0.f;
        p[k] = in ? a.pred[base + i] : 0.f;
    }
    uint32_t valid = 0;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const uint32_t i = i0 + k * NT;
        const int y = (int)(i / (uint32_t)a.W), x = (int)(i - (uint32_t)y * (uint32_t)a.W);
        const bool ok = i < (uint32_t)a.HW && g[k] > a.gt_lo && g[k] < a.gt_hi && y >= a.y1 && y < a.y2 && x >= a.x1 && x < a.x2;
        p[k] = clampf(p[k], a.c_lo, a.c_hi);
        valid |= (uint32_t)ok << k;
    }
    return valid;
}

// One count into h[digit] for every active lane.  ROUNDS > 0: lanes that hold the first active lane's digit are counted with
// a ballot and that lane adds the count, ROUNDS times; whatever is still active then adds 1 by itself.
template <int ROUNDS>
__device__ __forceinline__ void hist_add(uint32_t *h, bool active, uint32_t digit) {
    if (ROUNDS > 0) {
        const int lane = threadIdx.x & 63;
        unsigned long long todo = __ballot(active);
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            if (!todo) break;                                     // wave-uniform
            const int leader = __ffsll((long long)todo) - 1;
            const uint32_t ld = __shfl(digit, leader, 64);
            const unsigned long long same = __ballot(active && digit == ld);
            if (lane == leader) atomicAdd(&h[ld], (uint32_t)__popcll(same));
            if (digit == ld) active = false;
            todo &= ~same;
        }
    }
    if (active) atomicAdd(&h[digit], 1u);
}

struct Sel { uint32_t key[2], rank[2], n; };

// With histograms 0 .. K-1 of image b complete: find the digit of histogram K-1 that holds the wanted rank of both quantities
// and extend the keys by it.  All 256 threads call it, once per kernel; wsum / res are LDS scratch.
template <int K>
__device__ __forceinline__ Sel dm_resolve(const uint32_t *hist_b, uint32_t *state_b, uint32_t (*wsum)[4], uint32_t (*res)[2]) {
    constexpr int SHIFT = K == 1 ? 21 : (K == 2 ? 10 : 0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t *h = hist_b + (K - 1) * 2 * BINS;
    Sel s;
    uint32_t c[2][8], sum[2], excl[2];
    for (int q = 0; q < 2; ++q) {
        s.key[q] = K == 1 ? 0u : state_b[(K - 2) * 4 + q * 2];
        s.rank[q] = K == 1 ? 0u : state_b[(K - 2) * 4 + q * 2 + 1];
        sum[q] = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            c[q][j] = h[q * BINS + tid * 8 + j];
            sum[q] += c[q][j];
        }
        uint32_t inc = sum[q];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = __shfl_up(inc, off, 64);
            if (lane >= off) inc += v;
        }
        if (lane == 63) wsum[q][wave] = inc;
        excl[q] = inc - sum[q];
    }
    if (tid < 4) res[tid >> 1][tid & 1] = 0;
    __syncthreads();
    s.n = 0;
    for (int q = 0; q < 2; ++q) {
        uint32_t before = 0, total = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += wsum[q][w];
            total += wsum[q][w];
        }
        if (q == 0) s.n = total;
        const uint32_t rank = K == 1 ? (total ? (total - 1) / 2 : 0u) : s.rank[q];
        uint32_t lo = before + excl[q];
        if (total > 0 && rank >= lo && rank < lo + sum[q]) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (rank < lo + c[q][j]) {
                    res[q][0] = (uint32_t)(tid * 8 + j);
                    res[q][1] = rank - lo;
                    break;
                }
                lo += c[q][j];
            }
        }
    }
    __syncthreads();
    for (int q = 0; q < 2; ++q) {
        s.key[q] |= res[q][0] << SHIFT;
        s.rank[q] = res[q][1];
    }
    if (blockIdx.x == 0 && tid == 0) {
        for (int q = 0; q < 2; ++q) {
            state_b[(K - 1) * 4 + q * 2] = s.key[q];
            state_b[(K - 1) * 4 + q * 2 + 1] = s.rank[q];
        }
    }
    return s;
}

// Histograms and select state start every call from zero.  (A kernel, not hipMemsetAsync: the memset node of a captured
// graph left this region unzeroed on replay.)
__global__ __launch_bounds__(NT) void dm_zero_kernel(uint32_t *p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) p[i] = 0;
}

template <int PASS, int MODE>
__global__ __launch_bounds__(NT) void dm_hist_kernel(DmArgs a) {
    extern __shared__ uint32_t h[];                 // [copies][2][BINS]; copies = 4 (one per wave) in HIST_SUB, else 1
    __shared__ uint32_t wsum[2][4], res[2][2];
    constexpr int COPIES = MODE == HIST_SUB ? NT / 64 : 1;
    constexpr int ROUNDS = MODE == HIST_AGG ? AGG_ROUNDS : (MODE == HIST_AGG2 ? 2 : (MODE == HIST_AGG8 ? 8 : 0));
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < COPIES * 2 * BINS; i += NT) h[i] = 0;
    Sel s = {};
    if (PASS > 0) s = dm_resolve<PASS>(a.hist + (int64_t)b * HIST_U32, a.state + b * STATE_U32, wsum, res);
    __syncthreads();
    uint32_t *hw = h + (MODE == HIST_SUB ? (tid >> 6) * 2 * BINS : 0);
    const int64_t base = (int64_t)b * a.HW;
    float g[PPT], p[PPT];
    const uint32_t vmask = dm_load(a, base, blockIdx.x * (uint32_t)PPB + tid, g, p);
#pragma unroll
    for (int k = 0; k < PPT; ++k) {                  // no early exit: hist_add's ballots need whole waves
        const bool valid = (vmask >> k) & 1u;
        const uint32_t kg = __float_as_uint(g[k]), kp = __float_as_uint(p[k]);
        bool ag = valid, ap = valid;
        uint32_t dg = kg >> 21, dp = kp >> 21;
        if (PASS == 1) {
            ag = valid && dg == (s.key[0] >> 21);
            ap = valid && dp == (s.key[1] >> 21);
            dg = (kg >> 10) & 2047u;
            dp = (kp >> 10) & 2047u;
        } else if (PASS == 2) {
            ag = valid && (kg >> 10) == (s.key[0] >> 10);
            ap = valid && (kp >> 10) == (s.key[1] >> 10);
            dg = kg & 1023u;
            dp = kp & 1023u;
        }
        hist_add<ROUNDS>(hw, ag, dg);
        hist_add<ROUNDS>(hw + BINS, ap, dp);
    }
    __syncthreads();
    uint32_t *gh = a.hist + (int64_t)b * HIST_U32 + PASS * 2 * BINS;
    for (int i = tid; i < 2 * BINS; i += NT) {
        uint32_t v = h[i];
        for (int c = 1; c < COPIES; ++c) v += h[c * 2 * BINS + i];
        if (v) atomicAdd(&gh[i], v);
    }
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(NT) void dm_metrics_kernel(DmArgs a) {
    __shared__ uint32_t wsum[2][4], res[2][2], ired[5][4];
    __shared__ float red[5][4];
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
    const Sel s = dm_resolve<3>(a.hist + (int64_t)b * HIST_U32, a.state + b * STATE_U32, wsum, res);
    const bool scale_on = a.flags & DVF_DM_MEDIAN_SCALE, reclamp = a.flags & DVF_DM_RECLAMP;
    const float scale = __fdiv_rn(__uint_as_float(s.key[0]), __uint_as_float(s.key[1]));
    const int64_t base = (int64_t)b * a.HW;
    float f[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    uint32_t n[5] = {0, 0, 0, 0, 0};
    float gs[PPT], ps[PPT];
    const uint32_t vmask = dm_load(a, base, blockIdx.x * (uint32_t)PPB + tid, gs, ps);
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        if (!((vmask >> k) & 1u)) continue;
        const float g = gs[k];
        float p = ps[k];
        ++n[P_NVALID - 5];
        if (p != p) {
            ++n[P_NNAN - 5];
            continue;
        }
        if (scale_on) p = __fmul_rn(p, scale);
        if (reclamp) p = clampf(p, a.c_lo, a.c_hi);
        const float d = __fsub_rn(g, p), ad = fabsf(d), sq = __fmul_rn(d, d), dl = logf(g) - logf(p);
        f[P_ABS] += ad;
        f[P_REL] += __fdiv_rn(ad, g);
        f[P_SQREL] += __fdiv_rn(sq, g);
        f[P_SQ] += sq;
        f[P_LOGSQ] += __fmul_rn(dl, dl);
        const float ratio = fmaxf(__fdiv_rn(g, p), __fdiv_rn(p, g));
        n[P_A1 - 5] += ratio < 1.25f;
        n[P_A2 - 5] += ratio < 1.5625f;
        n[P_A3 - 5] += ratio < 1.953125f;
    }
    for (int c = 0; c < 5; ++c) {
        const float v = wave_sum(f[c]);
        const uint32_t m = wave_sum_u32(n[c]);
        if ((tid & 63) == 0) {
            red[c][wave] = v;
            ired[c][wave] = m;
        }
    }
    __syncthreads();
    if (tid < NPART) {
        float *P = a.partials + ((int64_t)b * a.nblk + blockIdx.x) * NPART;
        if (tid < 5) P[tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
        else P[tid] = __uint_as_float(ired[tid - 5][0] + ired[tid - 5][1] + ired[tid - 5][2] + ired[tid - 5][3]);
    }
}

// One block per image: the block partials added in index order (block_sum_strided), the counts as integers.
__global__ __launch_bounds__(NT) void dm_finish_kernel(DmArgs a) {
    __shared__ float red[4];
    __shared__ uint32_t ired[4];
    __shared__ float fs[5];
    __shared__ uint32_t is[5];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *P = a.partials + (int64_t)b * a.nblk * NPART;
    for (int c = 0; c < 5; ++c) {
        const float v = block_sum_strided(P, a.nblk, NPART, c, red);
        uint32_t m = 0;
        for (int i = tid; i < a.nblk; i += NT) m += __float_as_uint(P[(int64_t)i * NPART + 5 + c]);
        m = wave_sum_u32(m);
        if ((tid & 63) == 0) ired[tid >> 6] = m;
        __syncthreads();
        if (tid == 0) {
            fs[c] = v;
            is[c] = ired[0] + ired[1] + ired[2] + ired[3];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    float *o = a.out + b * 12;
    const uint32_t nv = is[P_NVALID - 5], nn = is[P_NNAN - 5];
    if (nv == 0) {
        for (int c = 0; c < 12; ++c) o[c] = 0.f;
        return;
    }
    const float inv = 1.f / (float)nv, nan = __uint_as_float(0x7fc00000u);
    const uint32_t *st = a.state + b * STATE_U32 + 2 * 4;
    o[0] = nn ? nan : fs[P_ABS] * inv;
    o[1] = nn ? nan : fs[P_REL] * inv;
    o[2] = nn ? nan : fs[P_SQREL] * inv;
    o[3] = nn ? nan : sqrtf(fs[P_SQ] * inv);
    o[4] = nn ? nan : sqrtf(fs[P_LOGSQ] * inv);
    for (int e = 0; e < 3; ++e) o[5 + e] = nn ? nan : (float)is[e] * inv;
    o[8] = (float)nv;
    o[9] = __uint_as_float(st[0]);
    o[10] = nn ? nan : __uint_as_float(st[2]);
    o[11] = (float)nn;
}

template <int MODE>
static int dm_launch_hist(const DmArgs &a, dim3 grid, hipStream_t st) {
    const size_t lds = (size_t)(MODE == HIST_SUB ? NT / 64 : 1) * 2 * BINS * sizeof(uint32_t);
#ifdef DVF_TUNING
    if (MODE == HIST_SUB) {   // 64 KiB of dynamic LDS next to the static scratch: above the default per-kernel limit
        static const hipError_t e[3] = {
            hipFuncSetAttribute((const void *)dm_hist_kernel<0, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
            hipFuncSetAttribute((const void *)dm_hist_kernel<1, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
            hipFuncSetAttribute((const void *)dm_hist_kernel<2, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)};
        if (e[0] != hipSuccess || e[1] != hipSuccess || e[2] != hipSuccess) return DVF_ERR_LAUNCH;
    }
#endif
    dm_hist_kernel<0, MODE><<<grid, NT, lds, st>>>(a);
    DVF_LAUNCH_CHECK();
    dm_hist_kernel<1, MODE><<<grid, NT, lds, st>>>(a);
    DVF_LAUNCH_CHECK();
    dm_hist_kernel<2, MODE><<<grid, NT, lds, st>>>(a);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

}  // namespace

extern "C" {

int64_t dvf_depth_metrics_ws_floats(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)B * (HIST_U32 + STATE_U32 + (int64_t)dm_blocks(H, W) * NPART);
}

int dvf_depth_metrics(const float *gt, const float *pred, float *out, float *ws, int64_t ws_floats, int B, int H, int W, int y1,
                      int y2, int x1, int x2, float gt_lo, float gt_hi, float clamp_lo, float clamp_hi, uint32_t flags,
                      void *stream) {
    if (!gt || !pred || !out || !ws || B <= 0 || H <= 0 || W <= 0 || B > 65535) return DVF_ERR_INVALID_ARG;
    if ((int64_t)B * H * W >= ((int64_t)1 << 31) || ws_floats < dvf_depth_metrics_ws_floats(B, H, W)) return DVF_ERR_INVALID_ARG;
    if (y1 < 0 || y1 > y2 || y2 > H || x1 < 0 || x1 > x2 || x2 > W) return DVF_ERR_INVALID_ARG;
    if (!(clamp_lo > 0.f) || !(clamp_lo <= clamp_hi) || !(gt_lo >= 0.f)) return DVF_ERR_INVALID_ARG;
    hipStream_t st = dvf_stream(stream);
    DmArgs a;
    a.gt = gt;
    a.pred = pred;
    a.hist = reinterpret_cast<uint32_t *>(ws);
    a.state = a.hist + (int64_t)B * HIST_U32;
    a.partials = ws + (int64_t)B * (HIST_U32 + STATE_U32);
    a.out = out;
    a.HW = H * W;
    a.W = W;
    a.y1 = y1, a.y2 = y2, a.x1 = x1, a.x2 = x2;
    a.nblk = dm_blocks(H, W);
    a.gt_lo = gt_lo, a.gt_hi = gt_hi, a.c_lo = clamp_lo, a.c_hi = clamp_hi;
    a.flags = flags;
    // (the partials are written in full by the metrics pass)
    const int64_t nzero = (int64_t)B * (HIST_U32 + STATE_U32);
    dm_zero_kernel<<<(int)((nzero + NT * 8 - 1) / (NT * 8) < 1024 ? (nzero + NT * 8 - 1) / (NT * 8) : 1024), NT, 0, st>>>(a.hist, nzero);
    DVF_LAUNCH_CHECK();
    const dim3 grid(a.nblk, B);
    int mode = HIST_AGG;
    if (const char *e = dvf_tune("DVF_DM_HIST")) mode = atoi(e);
    int rc;
#ifdef DVF_TUNING
    if (mode == HIST_DIRECT) rc = dm_launch_hist<HIST_DIRECT>(a, grid, st);
    else if (mode == HIST_SUB) rc = dm_launch_hist<HIST_SUB>(a, grid, st);
    else if (mode == HIST_AGG2) rc = dm_launch_hist<HIST_AGG2>(a, grid, st);
    else if (mode == HIST_AGG8) rc = dm_launch_hist<HIST_AGG8>(a, grid, st);
    else
#endif
        rc = dm_launch_hist<HIST_AGG>(a, grid, st);
    (void)mode;
    if (rc != DVF_OK) return rc;
    dm_metrics_kernel<<<grid, NT, 0, st>>>(a);
    DVF_LAUNCH_CHECK();
    dm_finish_kernel<<<B, NT, 0, st>>>(a);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

}  // extern "C"
