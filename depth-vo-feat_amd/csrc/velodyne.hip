// Ground-truth depth maps from LiDAR sweeps: the device form of generate_depth_map (tools/eval_depth_utils.py:172-224 of the
// reference) for a batch of frames.  Every point is projected in fp64, rounded to a pixel and the NEAREST point of a pixel
// wins; a pixel that no point reaches is 0.  Definition of every step: include/dvf_hip.h.
//
// The stored value max(d, 0) is a non-negative float, so its bit pattern orders as an unsigned integer and the per-pixel
// minimum is one integer atomicMin on the output buffer itself:
//   vd_fill_kernel     every pixel = EMPTY (0xffffffff, above every key: the largest key is +inf = 0x7f800000)
//   vd_scatter_kernel  one thread per point: project, round, bounds, atomicMin(pixel, bits of max(d, 0))
//   vd_finish_kernel   EMPTY -> 0; every other pixel already holds its float
// Clamping before the minimum equals the definition's minimum before the clamp (max(., 0) is monotone): one point of negative
// depth leaves key 0 and nothing undercuts it.  A minimum does not depend on arrival order: two runs are bit-identical.
// Traffic per frame: the sweep once (16 B a point), the map twice (fill, finish) plus one 4-byte atomic per kept point.
#include "dvf_common.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_BLOCKS = 2048;          // memory-bound passes: cap the grid and stride (256 CUs x 8 blocks)
constexpr uint32_t EMPTY = 0xffffffffu;

static inline int vd_grid(int64_t work) {
    const int64_t blocks = (work + NT - 1) / NT;
    return (int)(blocks < 1 ? 1 : (blocks > MAX_BLOCKS ? MAX_BLOCKS : blocks));
}

// keys[0 .. n): nvec 16-byte stores (keys is 16-byte aligned whenever nvec > 0), then the n - 4 * nvec elements of the tail
__global__ __launch_bounds__(NT) void vd_fill_kernel(uint32_t *keys, int64_t n, int64_t nvec) {
    const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x, step = (int64_t)gridDim.x * NT;
    uint4 *k4 = reinterpret_cast<uint4 *>(keys);
    for (int64_t i = t; i < nvec; i += step) k4[i] = make_uint4(EMPTY, EMPTY, EMPTY, EMPTY);
    for (int64_t i = 4 * nvec + t; i < n; i += step) keys[i] = EMPTY;
}

__global__ __launch_bounds__(NT) void vd_finish_kernel(uint32_t *keys, int64_t n, int64_t nvec) {
    const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x, step = (int64_t)gridDim.x * NT;
    uint4 *k4 = reinterpret_cast<uint4 *>(keys);
    for (int64_t i = t; i < nvec; i += step) {
        uint4 v = k4[i];
        v.x = v.x == EMPTY ? 0u : v.x;
        v.y = v.y == EMPTY ? 0u : v.y;
        v.z = v.z == EMPTY ? 0u : v.z;
        v.w = v.w == EMPTY ? 0u : v.w;
        k4[i] = v;
    }
    for (int64_t i = 4 * nvec + t; i < n; i += step)
        if (keys[i] == EMPTY) keys[i] = 0u;
}

// blockIdx.y walks the frames, blockIdx.x strides over the frame's own points.  offsets is device data nobody has checked:
// both ends of the range are clamped to [0, total] and a decreasing pair is an empty frame, so every index read lies in points.
__global__ __launch_bounds__(NT) void vd_scatter_kernel(const float4 *points, const int *offsets, const double *proj,
                                                        uint32_t *keys, int B, int H, int W, int total, uint32_t flags) {
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const int lo = min(max(offsets[b], 0), total), hi = min(max(offsets[b + 1], 0), total);
        const double *P = proj + (int64_t)b * 12;         // block-uniform, read once per frame
        const double p00 = P[0], p01 = P[1], p02 = P[2], p03 = P[3], p10 = P[4], p11 = P[5], p12 = P[6], p13 = P[7],
                     p20 = P[8], p21 = P[9], p22 = P[10], p23 = P[11];
        uint32_t *frame = keys + (int64_t)b * H * W;
        // (a decreasing pair: hi < lo and the loop does not run; lo + ... stays below 2^31 + 2^19 in 64 bits)
        for (int64_t i = (int64_t)lo + (int64_t)blockIdx.x * NT + threadIdx.x; i < hi; i += (int64_t)gridDim.x * NT) {
            const float4 q = points[i];                    // forward, left, up, reflectance (ignored: taken as 1)
            if (!(q.x >= 0.f)) continue;                   // behind the sensor, or NaN
            const double x = (double)q.x, y = (double)q.y, z = (double)q.z;
            const double c0 = fma(p00, x, fma(p01, y, fma(p02, z, p03)));
            const double c1 = fma(p10, x, fma(p11, y, fma(p12, z, p13)));
            const double c2 = fma(p20, x, fma(p21, y, fma(p22, z, p23)));
            const double u = rint(c0 / c2) - 1.0, v = rint(c1 / c2) - 1.0;     // half to even; KITTI's MATLAB offset
            if (!(u >= 0.0 && v >= 0.0 && u < (double)W && v < (double)H)) continue;   // NaN and +-inf (c2 == 0) fail
            const float d = (flags & DVF_VD_VELODYNE_DEPTH) ? q.x : (float)c2;
            const uint32_t key = d > 0.f ? __float_as_uint(d) : 0u;           // max(d, 0); -0 and NaN -> +0
            atomicMin(&frame[(int64_t)(int)v * W + (int)u], key);
        }
    }
}

}  // namespace

extern "C" {

int dvf_velodyne_depth(const float *points, const int *offsets, const double *proj, float *depth, int B, int H, int W, int total,
                       uint32_t flags, void *stream) {
    if (!offsets || !proj || !depth || B <= 0 || H <= 0 || W <= 0 || total < 0) return DVF_ERR_INVALID_ARG;
    if (!points && total != 0) return DVF_ERR_INVALID_ARG;
    if ((int64_t)B * H * W >= ((int64_t)1 << 31) || (flags & ~DVF_VD_VELODYNE_DEPTH)) return DVF_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(points) & 15) return DVF_ERR_INVALID_ARG;      // the kernel loads a point as one float4
    hipStream_t st = dvf_stream(stream);
    uint32_t *keys = reinterpret_cast<uint32_t *>(depth);
    const int64_t n = (int64_t)B * H * W;
    const int64_t nvec = (reinterpret_cast<uintptr_t>(depth) & 15) ? 0 : n / 4;
    const int pass_grid = vd_grid(nvec > 0 ? nvec : n);
    vd_fill_kernel<<<pass_grid, NT, 0, st>>>(keys, n, nvec);
    DVF_LAUNCH_CHECK();
    if (total > 0) {
        // no frame owns more than `total` points; blocks past a frame's own count leave at once
        const int gy = B < 65535 ? B : 65535, gx = vd_grid(total);
        vd_scatter_kernel<<<dim3(gx, gy), NT, 0, st>>>(reinterpret_cast<const float4 *>(points), offsets, proj, keys, B, H, W,
                                                       total, flags);
        DVF_LAUNCH_CHECK();
    }
    vd_finish_kernel<<<pass_grid, NT, 0, st>>>(keys, n, nvec);
    DVF_LAUNCH_CHECK();
    return DVF_OK;
}

}  // extern "C"
