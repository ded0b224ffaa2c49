// Odometry evaluation on the device: the chained camera-to-world trajectory of a sequence of relative poses and the KITTI
// segment errors of a trajectory against ground truth (odometry_eval.py's se3_cam2world / sequence_errors / overall_error;
// reference inference.py:63-70, tools/evaluation_tools.py:419-508), and, further down, the alignment of that trajectory to its
// ground truth with ATE, RPE and the snippet errors of inference.py:72-88.  Definition of every output: include/dvf_hip.h.
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

// the block's sum of acc[k] in a fixed tree; thread 0 returns with the totals in acc
template <int K>
__device__ __forceinline__ void block_sum(double (&acc)[K], double (*s)[NT]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) s[k][tid] = acc[k];
    __syncthreads();
    for (int d = NT / 2; d > 0; d >>= 1) {
        if (tid < d) {
#pragma unroll
            for (int k = 0; k < K; ++k) s[k][tid] += s[k][tid + d];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = s[k][0];
}

// thread 0 stores the block's K totals (block_sum's result) at the block's slot of part
template <int K>
__device__ __forceinline__ void store_block_totals(const double (&acc)[K], double *part) {
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 0; k < K; ++k) part[(int64_t)blockIdx.x * K + k] = acc[k];
}

// part[k] + part[stride + k] + ... over nb blocks, in block order
__device__ __forceinline__ double sum_in_block_order(const double *part, int nb, int stride, int k) {
    double m = 0.0;
    for (int b = 0; b < nb; ++b) m += part[(int64_t)b * stride + k];
    return m;
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
    block_sum<3>(acc, s);
    if (tid != 0) return;
    double path = 0.0;
    if (nrows > 0) path = dist[n - 1];
    else
        for (int i = 1; i < n; ++i) path += step_norm(gt, i);
#pragma unroll
    for (int c = 0; c < 3; ++c) summary[c] = accumulate ? summary[c] + acc[c] : acc[c];
    summary[3] = path;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Trajectory alignment and the errors of an aligned trajectory (odometry_eval.py's trajectory_alignment / apply_alignment /
// trajectory_errors / snippet_errors; reference inference.py:72-88 with the scale factor of :75).  The same rules: fp64, no
// atomics, every sum in a fixed order.  Sums over the frames are block partials (one 256-thread block per 256 frames, a fixed
// LDS tree) left in scratch, then added in block order:
//   align_sums_kernel      per block sum x (3), sum y (3), sum y.x, sum x.x of the translations x of res and y of gt
//   align_centred_kernel   the means from those partials in block order, then per block sum |x - mx|^2 and the nine entries of
//                          sum (y - my)(x - mx)^T: a second pass over the data, so a common offset of 1e6 m costs nothing
//   align_solve_kernel     one block adds the partials in block order, thread 0 solves the 3x3 problem and writes the record
//   apply_kernel           one thread per pose: [R R_i | c R t_i + t]
//   pair_errors_kernel / pair_finish_kernel        ATE and RPE
//   snippet_kernel / snippet_finish_kernel         one thread per start frame, the snippet's translations in registers
constexpr int ALIGN_NONE = 0, ALIGN_SCALE = 1, ALIGN_SCALE_7DOF = 2, ALIGN_6DOF = 3, ALIGN_7DOF = 4;
constexpr int SUMS = 8, CENTRED = 10, MAX_SNIPPET = 8;

__global__ __launch_bounds__(NT) void align_sums_kernel(const double *gt, const double *res, int n, double *part) {
    __shared__ double s[SUMS][NT];
    const int i = blockIdx.x * NT + threadIdx.x;
    double acc[SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < n) {
        const double *p = res + (int64_t)i * 12, *q = gt + (int64_t)i * 12;
        const double x[3] = {p[3], p[7], p[11]}, y[3] = {q[3], q[7], q[11]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc[k] = x[k];
            acc[3 + k] = y[k];
        }
        acc[6] = y[0] * x[0] + y[1] * x[1] + y[2] * x[2];
        acc[7] = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
    }
    block_sum<SUMS>(acc, s);
    store_block_totals<SUMS>(acc, part);
}

__global__ __launch_bounds__(NT) void align_centred_kernel(const double *gt, const double *res, int n, int nb, const double *part,
                                                           double *cpart) {
    __shared__ double s[CENTRED][NT];
    __shared__ double mean[6];
    if (threadIdx.x < 6) {                                             // mx, my: the partials in block order
        mean[threadIdx.x] = sum_in_block_order(part, nb, SUMS, threadIdx.x) / (double)n;
    }
    __syncthreads();
    const int i = blockIdx.x * NT + threadIdx.x;
    double acc[CENTRED] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < n) {
        const double *p = res + (int64_t)i * 12, *q = gt + (int64_t)i * 12;
        const double x[3] = {p[3] - mean[0], p[7] - mean[1], p[11] - mean[2]};
        const double y[3] = {q[3] - mean[3], q[7] - mean[4], q[11] - mean[5]};
        acc[0] = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[1 + r * 3 + c] = y[r] * x[c];
        }
    }
    block_sum<CENTRED>(acc, s);
    store_block_totals<CENTRED>(acc, cpart);
}

__device__ __forceinline__ void cross3(const double *a, const double *b, double *o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// a unit vector orthogonal to the unit vector u: u x (the axis u leans on least)
__device__ __forceinline__ void orthogonal_to(const double *u, double *o) {
    const int k = fabs(u[0]) <= fabs(u[1]) ? (fabs(u[0]) <= fabs(u[2]) ? 0 : 2) : (fabs(u[1]) <= fabs(u[2]) ? 1 : 2);
    double e[3] = {0.0, 0.0, 0.0};
    e[k] = 1.0;
    cross3(u, e, o);
    const double inv = 1.0 / sqrt(dot3(o, o));
    o[0] *= inv, o[1] *= inv, o[2] *= inv;
}

// The proper rotation R = U S V^T of M = U D V^T (S = diag(1, 1, sign(det U det V))), the singular values d (descending) and
// sign = S[2][2].  One-sided (Hestenes) Jacobi: plane rotations from the right make the columns of M orthogonal, M V = U D, at
// full relative accuracy (nothing is squared).  The rotation needs only the two leading pairs: with u2 = u0 x u1 and
// v2 = v0 x v1 the third term u2 v2^T IS sign * (third left vector)(third right vector)^T, so it is never divided out of a
// small column.  Rank 1 (a straight line): u1 is any unit vector orthogonal to u0; rank 0: the identity.
__device__ void polar3(const double *M, double *R, double *d, double *sign) {
    double g[3][3], v[3][3];                                           // columns: g[j] = M's column j, rotated; v[j] likewise
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            g[j][i] = M[i * 3 + j];
            v[j][i] = i == j ? 1.0 : 0.0;
        }
    }
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int pair = 0; pair < 3; ++pair) {
            const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2;
            const double a = dot3(g[p], g[p]), b = dot3(g[q], g[q]), c = dot3(g[p], g[q]);
            if (c == 0.0 || fabs(c) <= 2.3e-16 * sqrt(a * b)) continue;
            rotated = true;
            const double zeta = (b - a) / (2.0 * c);
            const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double gp = g[p][i], gq = g[q][i], vp = v[p][i], vq = v[q][i];
                g[p][i] = cs * gp - sn * gq;
                g[q][i] = sn * gp + cs * gq;
                v[p][i] = cs * vp - sn * vq;
                v[q][i] = sn * vp + cs * vq;
            }
        }
        if (!rotated) break;
    }
    double len[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) len[j] = sqrt(dot3(g[j], g[j]));
#pragma unroll
    for (int pair = 0; pair < 3; ++pair) {                             // descending: a three-element sorting network
        const int p = pair == 1 ? 1 : 0, q = pair == 1 ? 2 : 1;
        if (len[p] < len[q]) {
            const double l = len[p];
            len[p] = len[q];
            len[q] = l;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double gp = g[p][i], vp = v[p][i];
                g[p][i] = g[q][i], g[q][i] = gp;
                v[p][i] = v[q][i], v[q][i] = vp;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) d[j] = len[j];
    *sign = 1.0;
    if (!(len[0] > 0.0)) {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = i % 4 == 0 ? 1.0 : 0.0;
        return;
    }
    double u0[3], u1[3], u2[3], v2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) u0[i] = g[0][i] / len[0];
    if (len[1] > 1e-13 * len[0]) {
        // (one Gram-Schmidt step: R is orthonormal to rounding whatever the last sweep left)
        const double k = dot3(u0, g[1]);
        double w[3] = {g[1][0] - k * u0[0], g[1][1] - k * u0[1], g[1][2] - k * u0[2]};
        const double inv = 1.0 / sqrt(dot3(w, w));
#pragma unroll
        for (int i = 0; i < 3; ++i) u1[i] = w[i] * inv;
    } else {
        orthogonal_to(u0, u1);
    }
    cross3(u0, u1, u2);
    cross3(v[0], v[1], v2);
    // sign(det U det V): whether M maps v2 to the u2 side; a column of rounding noise (rank < 3) leaves +1 or -1, and either is
    // an optimal rotation then
    double mv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) mv[i] = M[i * 3] * v2[0] + M[i * 3 + 1] * v2[1] + M[i * 3 + 2] * v2[2];
    if (dot3(mv, u2) < 0.0) *sign = -1.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = u0[i] * v[0][j] + u1[i] * v[1][j] + u2[i] * v2[j];
    }
}

// record [16] = c, R[9], t[3], sv[3]
__global__ __launch_bounds__(64) void align_solve_kernel(const double *part, const double *cpart, int n, int nb, int mode,
                                                         double *record) {
    __shared__ double tot[SUMS + CENTRED];
    const int tid = threadIdx.x;
    if (mode != ALIGN_NONE && tid < SUMS + CENTRED) {
        double m = 0.0;
        if (tid < SUMS) m = sum_in_block_order(part, nb, SUMS, tid);
        else if (mode != ALIGN_SCALE) m = sum_in_block_order(cpart, nb, CENTRED, tid - SUMS);
        tot[tid] = m;
    }
    __syncthreads();
    if (tid != 0) return;
    double c = 1.0, R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0}, sv[3] = {0.0, 0.0, 0.0};
    if (mode == ALIGN_SCALE) {
        if (tot[7] != 0.0) c = tot[6] / tot[7];
    } else if (mode != ALIGN_NONE) {
        const double inv_n = 1.0 / (double)n, var = tot[SUMS] / (double)n;
        double M[9], rot[9], sign;
#pragma unroll
        for (int i = 0; i < 9; ++i) M[i] = tot[SUMS + 1 + i] / (double)n;
        polar3(M, rot, sv, &sign);
        const double c7 = var != 0.0 ? (sv[0] + sv[1] + sign * sv[2]) / var : 1.0;
        if (mode == ALIGN_SCALE_7DOF) {
            c = c7;
        } else {
            if (mode == ALIGN_7DOF) c = c7;
            const double mx[3] = {tot[0] * inv_n, tot[1] * inv_n, tot[2] * inv_n};
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = rot[i];
#pragma unroll
            for (int i = 0; i < 3; ++i)
                t[i] = tot[3 + i] * inv_n - c * (R[i * 3] * mx[0] + R[i * 3 + 1] * mx[1] + R[i * 3 + 2] * mx[2]);
        }
    }
    record[0] = c;
#pragma unroll
    for (int i = 0; i < 9; ++i) record[1 + i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        record[10 + i] = t[i];
        record[13 + i] = sv[i];
    }
}

__global__ __launch_bounds__(NT) void apply_kernel(const double *res, const double *record, int n, int copy, double *out) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const Rigid p = load_pose(res + (int64_t)i * 12);
    if (copy) {
        store_pose(out + (int64_t)i * 12, p);
        return;
    }
    const double c = record[0];
    Rigid a;
#pragma unroll
    for (int k = 0; k < 9; ++k) a.r[k] = record[1 + k];
    a.t[0] = a.t[1] = a.t[2] = 0.0;
    Rigid o = compose(a, p);                                           // [R R_i | R t_i]
#pragma unroll
    for (int k = 0; k < 3; ++k) o.t[k] = c * o.t[k] + record[10 + k];
    store_pose(out + (int64_t)i * 12, o);
}

// atan2(|skew part|, trace - 1): the angle form of compute_pose_error (inference.py:82-86), exact down to zero
__device__ __forceinline__ double rotation_angle(const double *r) {
    const double a = r[1] - r[3], b = r[5] - r[7], c = r[2] - r[6];
    return atan2(sqrt(a * a + b * b + c * c), r[0] + r[4] + r[8] - 1.0);
}

__global__ __launch_bounds__(NT) void pair_errors_kernel(const double *gt, const double *res, int n, double *part) {
    __shared__ double s[3][NT];
    const int i = blockIdx.x * NT + threadIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};
    if (i < n) {
        const Rigid g = load_pose(gt + (int64_t)i * 12), r = load_pose(res + (int64_t)i * 12);
        const double dx = g.t[0] - r.t[0], dy = g.t[1] - r.t[1], dz = g.t[2] - r.t[2];
        acc[0] = dx * dx + dy * dy + dz * dz;
        if (i + 1 < n) {
            const Rigid d_gt = compose(inverse(g), load_pose(gt + (int64_t)(i + 1) * 12));
            const Rigid d_res = compose(inverse(r), load_pose(res + (int64_t)(i + 1) * 12));
            const Rigid e = compose(inverse(d_gt), d_res);
            acc[1] = sqrt(e.t[0] * e.t[0] + e.t[1] * e.t[1] + e.t[2] * e.t[2]);
            acc[2] = rotation_angle(e.r);
        }
    }
    block_sum<3>(acc, s);
    store_block_totals<3>(acc, part);
}

// out [4] = [ate, rpe_trans, rpe_rot, n]
__global__ __launch_bounds__(64) void pair_finish_kernel(const double *part, int n, int nb, double *out) {
    __shared__ double tot[3];
    const int tid = threadIdx.x;
    if (tid < 3) tot[tid] = sum_in_block_order(part, nb, 3, tid);
    __syncthreads();
    if (tid != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    out[0] = sqrt(tot[0] / (double)n);
    out[1] = n > 1 ? tot[1] / (double)(n - 1) : nan;
    out[2] = n > 1 ? tot[2] / (double)(n - 1) : nan;
    out[3] = (double)n;
}

__global__ __launch_bounds__(NT) void snippet_kernel(const double *gt, const double *res, int nrows, int length, double *rows,
                                                     double *part) {
    __shared__ double s[3][NT];
    const int i = blockIdx.x * NT + threadIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};
    if (i < nrows) {
        const Rigid g0 = inverse(load_pose(gt + (int64_t)i * 12)), p0 = inverse(load_pose(res + (int64_t)i * 12));
        double gt_t[MAX_SNIPPET][3], pr_t[MAX_SNIPPET][3];
        double gp = 0.0, pp = 0.0, angle = 0.0;
#pragma unroll
        for (int k = 0; k < MAX_SNIPPET; ++k) {
            if (k < length) {
                const Rigid g = compose(g0, load_pose(gt + (int64_t)(i + k) * 12));
                const Rigid p = compose(p0, load_pose(res + (int64_t)(i + k) * 12));
                Rigid pr = p;
                pr.t[0] = pr.t[1] = pr.t[2] = 0.0;
                Rigid gr = g;
                gr.t[0] = gr.t[1] = gr.t[2] = 0.0;
                const Rigid e = compose(gr, inverse(pr));              // R_gt inv(R_pred)
                angle += rotation_angle(e.r);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    gt_t[k][c] = g.t[c];
                    pr_t[k][c] = p.t[c];
                }
                gp += g.t[0] * p.t[0] + g.t[1] * p.t[1] + g.t[2] * p.t[2];
                pp += p.t[0] * p.t[0] + p.t[1] * p.t[1] + p.t[2] * p.t[2];
            }
        }
        const double scale = pp != 0.0 ? gp / pp : 1.0;
        double sq = 0.0;
#pragma unroll
        for (int k = 0; k < MAX_SNIPPET; ++k) {
            if (k < length) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double d = gt_t[k][c] - scale * pr_t[k][c];
                    sq += d * d;
                }
            }
        }
        const double ate = sqrt(sq) / (double)length, re = angle / (double)length;
        rows[(int64_t)i * 2] = ate;
        rows[(int64_t)i * 2 + 1] = re;
        acc[0] = ate;
        acc[1] = ate * ate;
        acc[2] = re;
    }
    block_sum<3>(acc, s);
    store_block_totals<3>(acc, part);
}

// summary [5] = [sum ate, sum ate^2, sum re, rows, 0]
__global__ __launch_bounds__(64) void snippet_finish_kernel(const double *part, int nrows, int nb, int accumulate, double *summary) {
    const int tid = threadIdx.x;
    if (tid < 3) {
        const double m = sum_in_block_order(part, nb, 3, tid);
        summary[tid] = accumulate ? summary[tid] + m : m;
    } else if (tid == 3) {
        summary[3] = accumulate ? summary[3] + (double)nrows : (double)nrows;
    } else if (tid == 4) {
        summary[4] = 0.0;
    }
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

int64_t dvf_trajectory_align_ws_doubles(int n) { return n < 1 ? 0 : (int64_t)cdiv(n, NT) * (SUMS + CENTRED); }

int dvf_trajectory_align(const double *gt, const double *res, int n, int mode, double *transform, double *ws, int64_t ws_doubles,
                         void *stream) {
    if (n < 1 || n >= (1 << 24) || !gt || !res || !transform || !ws || ws_doubles < dvf_trajectory_align_ws_doubles(n))
        return DVF_ERR_INVALID_ARG;
    if (mode < ALIGN_NONE || mode > ALIGN_7DOF) return DVF_ERR_INVALID_ARG;
    const bool centred = mode == ALIGN_SCALE_7DOF || mode == ALIGN_6DOF || mode == ALIGN_7DOF;
    if (centred && n < 3) return DVF_ERR_INVALID_ARG;
    hipStream_t st = dvf_stream(stream);
    const int nb = cdiv(n, NT);
    double *part = ws, *cpart = ws + (int64_t)nb * SUMS;
    if (mode != ALIGN_NONE) {
        align_sums_kernel<<<nb, NT, 0, st>>>(gt, res, n, part);
        DVF_LAUNCH_CHECK();
    }
    if (centred) {
        align_centred_kernel<<<nb, NT, 0, st>>>(gt, res, n, nb, part, cpart);
        DVF_LAUNCH_CHECK();
    }
    align_solve_kernel<<<1, 64, 0, st>>>(part, cpart, n, nb, mode, transform);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

int dvf_trajectory_apply(const double *res, const double *transform, int n, int copy, double *out, void *stream) {
    if (n < 1 || n >= (1 << 24) || !res || !out || (!copy && !transform)) return DVF_ERR_INVALID_ARG;
    apply_kernel<<<cdiv(n, NT), NT, 0, dvf_stream(stream)>>>(res, transform, n, copy, out);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

int64_t dvf_trajectory_errors_ws_doubles(int n) { return n < 1 ? 0 : (int64_t)cdiv(n, NT) * 3; }

int dvf_trajectory_errors(const double *gt, const double *res, int n, double *out, double *ws, int64_t ws_doubles, void *stream) {
    if (n < 1 || n >= (1 << 24) || !gt || !res || !out || !ws || ws_doubles < dvf_trajectory_errors_ws_doubles(n))
        return DVF_ERR_INVALID_ARG;
    hipStream_t st = dvf_stream(stream);
    const int nb = cdiv(n, NT);
    pair_errors_kernel<<<nb, NT, 0, st>>>(gt, res, n, ws);
    DVF_LAUNCH_CHECK();
    pair_finish_kernel<<<1, 64, 0, st>>>(ws, n, nb, out);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

int64_t dvf_snippet_errors_ws_doubles(int n) { return n < 1 ? 0 : (int64_t)cdiv(n, NT) * 3; }

int dvf_snippet_errors(const double *gt, const double *res, int n, int length, double *rows, double *summary, int accumulate,
                       double *ws, int64_t ws_doubles, void *stream) {
    if (n < 1 || n >= (1 << 24) || length < 2 || length > MAX_SNIPPET || !gt || !res || !summary || !ws ||
        ws_doubles < dvf_snippet_errors_ws_doubles(n))
        return DVF_ERR_INVALID_ARG;
    const int nrows = n >= length ? n - length + 1 : 0, nb = cdiv(nrows, NT);
    if (nrows > 0 && !rows) return DVF_ERR_INVALID_ARG;
    hipStream_t st = dvf_stream(stream);
    if (nrows > 0) {
        snippet_kernel<<<nb, NT, 0, st>>>(gt, res, nrows, length, rows, ws);
        DVF_LAUNCH_CHECK();
    }
    snippet_finish_kernel<<<1, 64, 0, st>>>(ws, nrows, nb, accumulate, summary);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

}  // extern "C"
