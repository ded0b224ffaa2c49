// Odometry evaluation on the device: the chained camera-to-world trajectory of a sequence of relative poses and the KITTI
// segment errors of a trajectory against ground truth (odometry_eval.py's se3_cam2world / sequence_errors / overall_error;
// reference inference.py:63-70, tools/evaluation_tools.py:419-508).  Definition of every output: include/dvf_hip.h.
//
// Everything is fp64 and every kernel is a latency problem (a KITTI sequence has at most 4541 poses), so the shapes are
// chosen for few dependent steps, not for throughput:
//   chain_kernel     one 256-thread block per sequence.  A transform is (R, t), 12 doubles, and the chain is an inclusive scan
//                    over (A * B) = (Ra Rb, Ra tb + ta), associative but not commutative: the EARLIER element is always the
//                    left operand.  Thread t multiplies its contiguous chunk in order, the 256 chunk products are scanned
//                    through LDS (Hillis-Steele, 8 steps, 24 KB), and a second pass over the chunk starts from the exclusive
//                    prefix and writes the poses.
//   dist_kernel      one block: step norms of the ground truth, the same chunk / scan / second-pass shape over a plain sum.
//   rows_kernel      one thread per (start frame, segment length): binary search of the segment end in dist, then the error.
//   summary_kernel   one block: per-thread partial sums over the rows in a strided order, a fixed tree through LDS.
// No float atomic anywhere: two runs are bit-identical.
#include "dvf_common.h"

namespace {

constexpr int NT = 256, MAX_SEQ = 32, NLEN = 8, FIRST_FRAME = 9, FRAME_STEP = 10, ROW = 6;
constexpr double FRAME_PERIOD = 0.1;   // 10 Hz, the speed constant of evaluation_tools.py:482

struct Rigid { double r[9], t[3]; };

__device__ __forceinline__ Rigid rigid_identity() {
    Rigid a;
#pragma unroll
    for (int i = 0; i < 9; ++i) a.r[i] = (i % 4 == 0) ? 1.0 : 0.0;
    a.t[0] = a.t[1] = a.t[2] = 0.0;
    return a;
}

// a * b: a is applied last (the left factor of the matrix product)
__device__ __forceinline__ Rigid compose(const Rigid &a, const Rigid &b) {
    Rigid c;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) c.r[i * 3 + j] = a.r[i * 3] * b.r[j] + a.r[i * 3 + 1] * b.r[3 + j] + a.r[i * 3 + 2] * b.r[6 + j];
        c.t[i] = a.r[i * 3] * b.t[0] + a.r[i * 3 + 1] * b.t[1] + a.r[i * 3 + 2] * b.t[2] + a.t[i];
    }
    return c;
}

// inverse of the affine [A|t]: (A^-1, -A^-1 t), A^-1 by cofactors (the transpose when A is orthonormal)
__device__ __forceinline__ Rigid inverse(const Rigid &a) {
    const double *m = a.r;
    double c[9];
    c[0] = m[4] * m[8] - m[5] * m[7];
    c[1] = m[2] * m[7] - m[1] * m[8];
    c[2] = m[1] * m[5] - m[2] * m[4];
    c[3] = m[5] * m[6] - m[3] * m[8];
    c[4] = m[0] * m[8] - m[2] * m[6];
    c[5] = m[2] * m[3] - m[0] * m[5];
    c[6] = m[3] * m[7] - m[4] * m[6];
    c[7] = m[1] * m[6] - m[0] * m[7];
    c[8] = m[0] * m[4] - m[1] * m[3];
    const double inv_det = 1.0 / (m[0] * c[0] + m[1] * c[3] + m[2] * c[6]);
    Rigid o;
#pragma unroll
    for (int i = 0; i < 9; ++i) o.r[i] = c[i] * inv_det;
#pragma unroll
    for (int i = 0; i < 3; ++i) o.t[i] = -(o.r[i * 3] * a.t[0] + o.r[i * 3 + 1] * a.t[1] + o.r[i * 3 + 2] * a.t[2]);
    return o;
}

__device__ __forceinline__ Rigid load_rel(const float *p) {   // rows 0..2 of a [4][4] fp32 matrix
    Rigid a;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) a.r[i * 3 + j] = (double)p[i * 4 + j];
        a.t[i] = (double)p[i * 4 + 3];
    }
    return a;
}

__device__ __forceinline__ Rigid load_pose(const double *p) {   // a [3][4] fp64 pose
    Rigid a;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) a.r[i * 3 + j] = p[i * 4 + j];
        a.t[i] = p[i * 4 + 3];
    }
    return a;
}

__device__ __forceinline__ void store_pose(double *p, const Rigid &a) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) p[i * 4 + j] = a.r[i * 3 + j];
        p[i * 4 + 3] = a.t[i];
    }
}

// component-major LDS image of 256 transforms: lane t reads word t of every component, no bank conflict
__device__ __forceinline__ void lds_put(double (*s)[NT], int t, const Rigid &a) {
#pragma unroll
    for (int i = 0; i < 9; ++i) s[i][t] = a.r[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) s[9 + i][t] = a.t[i];
}

__device__ __forceinline__ Rigid lds_get(double (*s)[NT], int t) {
    Rigid a;
#pragma unroll
    for (int i = 0; i < 9; ++i) a.r[i] = s[i][t];
#pragma unroll
    for (int i = 0; i < 3; ++i) a.t[i] = s[9 + i][t];
    return a;
}

struct ChainArgs {
    const float *rel;
    double *world;
    int off[MAX_SEQ + 1];
};

__global__ __launch_bounds__(NT) void chain_kernel(ChainArgs a) {
    __shared__ double s[12][NT];
    const int seq = blockIdx.x, tid = threadIdx.x;
    const int begin = a.off[seq], n = a.off[seq + 1] - begin;
    const int chunk = (n + NT - 1) / NT;
    const int k0 = min(tid * chunk, n), k1 = min(k0 + chunk, n);       // this thread's elements [k0, k1) of the sequence
    const float *rel = a.rel + (int64_t)begin * 16;
    double *world = a.world + ((int64_t)begin + seq) * 12;            // row offsets[s] + s
    Rigid acc = rigid_identity();
    for (int k = k0; k < k1; ++k) acc = compose(acc, load_rel(rel + (int64_t)k * 16));
    lds_put(s, tid, acc);
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {                                 // inclusive scan: s[t] = s[t - d] * s[t], earlier on the left
        Rigid left;
        if (tid >= d) left = lds_get(s, tid - d);
        __syncthreads();
        if (tid >= d) {
            acc = compose(left, acc);
            lds_put(s, tid, acc);
        }
        __syncthreads();
    }
    Rigid T = tid > 0 ? lds_get(s, tid - 1) : rigid_identity();        // product of everything before this chunk
    if (tid == 0) store_pose(world, T);
    for (int k = k0; k < k1; ++k) {
        T = compose(T, load_rel(rel + (int64_t)k * 16));
        store_pose(world + ((int64_t)k + 1) * 12, T);
    }
}

__device__ __forceinline__ double step_norm(const double *gt, int i) {   // |t_i - t_{i-1}|, i >= 1
    const double *p = gt + (int64_t)i * 12, *q = p - 12;
    const double dx = p[3] - q[3], dy = p[7] - q[7], dz = p[11] - q[11];
    return sqrt(dx * dx + dy * dy + dz * dz);
}

// dist[0] = 0, dist[i] = dist[i - 1] + |t_i - t_{i-1}|
__global__ __launch_bounds__(NT) void dist_kernel(const double *gt, int n, double *dist) {
    __shared__ double s[NT];
    const int tid = threadIdx.x;
    const int m = n - 1, chunk = (m + NT - 1) / NT;                    // m steps, step k ends at frame k + 1
    const int k0 = min(tid * chunk, m), k1 = min(k0 + chunk, m);
    double acc = 0.0;
    for (int k = k0; k < k1; ++k) acc += step_norm(gt, k + 1);
    s[tid] = acc;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        const double left = tid >= d ? s[tid - d] : 0.0;
        __syncthreads();
        if (tid >= d) {
            acc = left + acc;
            s[tid] = acc;
        }
        __syncthreads();
    }
    double run = tid > 0 ? s[tid - 1] : 0.0;
    if (tid == 0) dist[0] = 0.0;
    for (int k = k0; k < k1; ++k) {
        run += step_norm(gt, k + 1);
        dist[k + 1] = run;
    }
}

__global__ __launch_bounds__(NT) void rows_kernel(const double *gt, const double *res, const double *dist, int n, int nrows,
                                                  double *rows) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= nrows) return;
    const int first = FIRST_FRAME + FRAME_STEP * (i / NLEN);
    const double length = 100.0 * (double)(i % NLEN + 1);
    double *row = rows + (int64_t)i * ROW;
    const double limit = dist[first] + length;
    int lo = first + 1, hi = n;                                        // the first index in (first, n) with dist > limit; n if none
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (dist[mid] > limit) hi = mid;
        else lo = mid + 1;
    }
    if (lo >= n) {
#pragma unroll
        for (int c = 0; c < ROW; ++c) row[c] = 0.0;
        return;
    }
    const int last = lo;
    const Rigid d_gt = compose(inverse(load_pose(gt + (int64_t)first * 12)), load_pose(gt + (int64_t)last * 12));
    const Rigid d_res = compose(inverse(load_pose(res + (int64_t)first * 12)), load_pose(res + (int64_t)last * 12));
    const Rigid e = compose(inverse(d_res), d_gt);
    const double c = 0.5 * (e.r[0] + e.r[4] + e.r[8] - 1.0);
    const double r_err = acos(fmin(fmax(c, -1.0), 1.0));
    const double t_err = sqrt(e.t[0] * e.t[0] + e.t[1] * e.t[1] + e.t[2] * e.t[2]);
    row[0] = (double)first;
    row[1] = r_err / length;
    row[2] = t_err / length;
    row[3] = length;
    row[4] = length / (FRAME_PERIOD * ((double)(last - first) + 1.0));
    row[5] = 1.0;
}

// summary = [sum t_err/L, sum r_err/L, rows, path length].  With no row (n <= 9) no dist exists: thread 0 walks the few steps.
__global__ __launch_bounds__(NT) void summary_kernel(const double *gt, const double *rows, const double *dist, int n, int nrows,
                                                     int accumulate, double *summary) {
    __shared__ double s[3][NT];
    const int tid = threadIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < nrows; i += NT) {
        const double *row = rows + (int64_t)i * ROW;
        acc[0] += row[2];
        acc[1] += row[1];
        acc[2] += row[5];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c][tid] = acc[c];
    __syncthreads();
    for (int d = NT / 2; d > 0; d >>= 1) {
        if (tid < d) {
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c][tid] += s[c][tid + d];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    double path = 0.0;
    if (nrows > 0) path = dist[n - 1];
    else
        for (int i = 1; i < n; ++i) path += step_norm(gt, i);
#pragma unroll
    for (int c = 0; c < 3; ++c) summary[c] = accumulate ? summary[c] + s[c][0] : s[c][0];
    summary[3] = path;
}

}  // namespace

extern "C" {

int dvf_pose_chain(const float *rel, const int *offsets, int S, double *world, void *stream) {
    if (!rel || !offsets || !world || S < 1 || S > MAX_SEQ) return DVF_ERR_INVALID_ARG;
    ChainArgs a;
    a.rel = rel;
    a.world = world;
    if (offsets[0] != 0) return DVF_ERR_INVALID_ARG;
    for (int s = 0; s <= MAX_SEQ; ++s) a.off[s] = offsets[s < S ? s : S];
    for (int s = 0; s < S; ++s)
        if (a.off[s + 1] < a.off[s]) return DVF_ERR_INVALID_ARG;
    if (a.off[S] >= (1 << 24)) return DVF_ERR_INVALID_ARG;
    chain_kernel<<<S, NT, 0, dvf_stream(stream)>>>(a);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

int64_t dvf_odometry_errors_ws_doubles(int n) { return n < 1 ? 0 : (int64_t)n; }

int dvf_odometry_errors(const double *gt, const double *res, int n, double *rows, double *summary, int accumulate, double *ws,
                        int64_t ws_doubles, void *stream) {
    if (n < 1 || !gt || !res || !summary || !ws || ws_doubles < dvf_odometry_errors_ws_doubles(n)) return DVF_ERR_INVALID_ARG;
    const int nstart = n > FIRST_FRAME ? (n - FIRST_FRAME + FRAME_STEP - 1) / FRAME_STEP : 0, nrows = nstart * NLEN;
    if (nrows > 0 && !rows) return DVF_ERR_INVALID_ARG;
    hipStream_t st = dvf_stream(stream);
    if (nrows > 0) {
        dist_kernel<<<1, NT, 0, st>>>(gt, n, ws);
        DVF_LAUNCH_CHECK();
        rows_kernel<<<cdiv(nrows, NT), NT, 0, st>>>(gt, res, ws, n, nrows, rows);
        DVF_LAUNCH_CHECK();
    }
    summary_kernel<<<1, NT, 0, st>>>(gt, rows, ws, n, nrows, accumulate, summary);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

}  // extern "C"
