// Host-side description of one convolution-shaped op -- a forward, or the dgrad of one input segment -- from which both
// the pipelined route (conv_pipe_host.h) and the gather route (conv.hip) plan their launch.
#pragma once
#include "dvf_common.h"
#include "conv_head.h"

namespace {

inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
inline int roundup(int v, int q) { return (v + q - 1) / q * q; }

// One class of output pixels (oy*OS+py, ox*OS+px) that read the input pixels (oy*IS+by+ta, ox*IS+bx+tb), ta < TA, tb < TB;
// class tap t is tap tapmap[t] of the stored kernel.
struct ClassSpec { int OS, py, px, IS, by, bx, TA, TB, OHc, OWc; int tapmap[49]; };

// One op = one (M range, reduction segments, classes) triple.  Geometry only: the operands arrive at launch (ConvIO).
struct ConvOp {
    int nseg, segC[DVF_MAX_SEGS];        // reduction segments (virtual concatenation)
    int w_mode;                          // 0: w[((m_base+m)*Rtot + r)*KK + tap]   1: w[(r*Mtot + m_base+m)*KK + tap]
    int Mtot, Rtot, KK, m_base, M;
    int N, IH, IW, OH, OW;
    int act;                             // epilogue: out = act(sum + bias)
    float alpha, beta;
    ClassSpec cls[4];                    // the classes share one launch
    int ncls;
    bool covers;                         // the classes cover every output pixel
    int Tmax, TAmax, TBmax, OHc, OWc;    // maxima over the classes
    bool head_fwd;                       // forward of a Conv2d head: the 1-4 channel heads over >= 128 channels may run pipelined
};

struct ConvIO {
    const float *const *in;              // nseg tensors [N, segC[s], IH, IW]
    const float *bias;                   // indexed by m, or NULL
    float *out;                          // [N, M, OH, OW]
    const float *mask;                   // dgrad of a segment produced by a ReLU layer: out = (mask > 0) ? v : 0, or NULL
};

int check_desc(const dvf_conv_desc *d) {
    if (!d) return DVF_ERR_INVALID_ARG;
    if (d->N <= 0 || d->C_in <= 0 || d->C_out <= 0 || d->H_in <= 0 || d->W_in <= 0 || d->H_out <= 0 || d->W_out <= 0)
        return DVF_ERR_INVALID_ARG;
    if (d->KH < 1 || d->KW < 1 || d->KH > 7 || d->KW > 7 || (d->stride != 1 && d->stride != 2) || d->pad < 0)
        return DVF_ERR_INVALID_ARG;
    return DVF_OK;
}

int check_segs(const dvf_conv_desc *d, const int *seg_channels, int nseg) {
    if (nseg < 1 || nseg > DVF_MAX_SEGS || !seg_channels) return DVF_ERR_INVALID_ARG;
    int tot = 0;
    for (int s = 0; s < nseg; ++s) {
        if (seg_channels[s] <= 0) return DVF_ERR_INVALID_ARG;
        tot += seg_channels[s];
    }
    return tot == d->C_in ? DVF_OK : DVF_ERR_INVALID_ARG;
}

// Taps of output-parity class `c` for the relation  Y = o*S - pad + a  <=>  o = (Y + pad - a) / S.
// Taps are listed so that o = (Y - c)/S + base + index.  Returns the tap count.
int class_taps(int c, int S, int pad, int K, int *taps, int *base) {
    int amax = -1;
    for (int a = K - 1; a >= 0; --a)
        if ((c + pad - a) % S == 0) { amax = a; break; }
    if (amax < 0) { *base = 0; return 0; }
    int cnt = 0;
    for (int a = amax; a >= 0; a -= S) taps[cnt++] = a;
    *base = (c + pad - amax) / S;     // exact division (possibly negative)
    return cnt;
}

// classes of the scatter relation for an output of size OHxOW
int scatter_classes(int S, int pad, int KH, int KW, int OH, int OW, ClassSpec *cls, bool *covers_all) {
    int n = 0;
    *covers_all = true;
    for (int cy = 0; cy < S; ++cy)
        for (int cx = 0; cx < S; ++cx) {
            int ta[7], tb[7], by, bx;
            const int na = class_taps(cy, S, pad, KH, ta, &by), nb = class_taps(cx, S, pad, KW, tb, &bx);
            const int OHc = (OH - cy + S - 1) / S, OWc = (OW - cx + S - 1) / S;
            if (OHc <= 0 || OWc <= 0) continue;
            if (na == 0 || nb == 0) { *covers_all = false; continue; }
            ClassSpec &c = cls[n++];
            c = ClassSpec{S, cy, cx, 1, by, bx, na, nb, OHc, OWc, {0}};
            for (int i = 0; i < na; ++i)
                for (int j = 0; j < nb; ++j) c.tapmap[i * nb + j] = ta[i] * KW + tb[j];
        }
    // heaviest class first (longest-processing-time order: a launch dispatches its classes in this order, class-major, so the
    // 4-tap blocks of a 3x3 stride-2 launch start first and the 1-tap blocks fill the tail -- conv_pipe.h, blockIdx.z)
    for (int i = 1; i < n; ++i)
        for (int j = i; j > 0 && cls[j].TA * cls[j].TB > cls[j - 1].TA * cls[j - 1].TB; --j) {
            const ClassSpec t = cls[j]; cls[j] = cls[j - 1]; cls[j - 1] = t;
        }
    return n;
}

// Classes of `op` for the relation between its OHxOW output and its input: the gather relation (one class, the identity
// tap map) or the scatter relation (output-parity classes).  DVF_ERR_UNSUPPORTED when no class has a tap.
int set_classes(const dvf_conv_desc *d, bool gather, ConvOp &op) {
    if (gather) {
        op.ncls = 1; op.covers = true;
        op.cls[0] = ClassSpec{1, 0, 0, d->stride, -d->pad, -d->pad, d->KH, d->KW, op.OH, op.OW, {0}};
        for (int t = 0; t < op.KK; ++t) op.cls[0].tapmap[t] = t;
    } else {
        op.ncls = scatter_classes(d->stride, d->pad, d->KH, d->KW, op.OH, op.OW, op.cls, &op.covers);
    }
    op.Tmax = op.TAmax = op.TBmax = op.OHc = op.OWc = 0;
    for (int i = 0; i < op.ncls; ++i) {
        const ClassSpec &c = op.cls[i];
        op.Tmax = max(op.Tmax, c.TA * c.TB); op.TAmax = max(op.TAmax, c.TA); op.TBmax = max(op.TBmax, c.TB);
        op.OHc = max(op.OHc, c.OHc); op.OWc = max(op.OWc, c.OWc);
    }
    return op.ncls >= 1 ? DVF_OK : DVF_ERR_UNSUPPORTED;
}

// Forward:
//   Conv2d           out[co][oy][ox] = sum_ci sum_ab W[co][ci][a][b] * in[ci][oy*s - p + a][ox*s - p + b]
//   ConvTranspose2d  out[co][Y][X]   = sum_ci sum_ab W[ci][co][a][b] * in[ci][i][j],  Y = i*s - p + a
int make_fwd_op(const dvf_conv_desc *d, const int *seg_channels, int nseg, ConvOp &op) {
    op = ConvOp{};
    for (int s = 0; s < nseg; ++s) op.segC[s] = seg_channels[s];
    op.nseg = nseg; op.M = d->C_out;
    op.N = d->N; op.IH = d->H_in; op.IW = d->W_in; op.OH = d->H_out; op.OW = d->W_out;
    op.act = d->act; op.alpha = d->alpha; op.beta = d->beta;
    op.KK = d->KH * d->KW; op.m_base = 0; op.Mtot = d->C_out; op.Rtot = d->C_in;
    op.head_fwd = !dvf_head_fwd_applicable(d, nseg) && dvf_head_applicable(d, nseg);
    op.w_mode = d->transposed ? 1 : 0;
    return set_classes(d, !d->transposed, op);
}

// dgrad of the input segment of `segc` channels at channel `off`:
//   Conv2d           din[ci][Y][X] = sum_co sum_ab W[co][ci][a][b] * dpre[co][o][..],  Y = o*s - p + a
//   ConvTranspose2d  din[ci][i][j] = sum_co sum_ab W[ci][co][a][b] * dpre[co][i*s - p + a][j*s - p + b]
int make_dgrad_op(const dvf_conv_desc *d, int off, int segc, ConvOp &op) {
    op = ConvOp{};
    op.segC[0] = d->C_out; op.nseg = 1; op.M = segc;
    op.N = d->N; op.IH = d->H_out; op.IW = d->W_out; op.OH = d->H_in; op.OW = d->W_in;
    op.act = DVF_ACT_NONE;
    op.KK = d->KH * d->KW; op.m_base = off; op.Mtot = d->C_in; op.Rtot = d->C_out;
    op.head_fwd = false;
    op.w_mode = d->transposed ? 0 : 1;
    return set_classes(d, d->transposed != 0, op);
}

}  // namespace
