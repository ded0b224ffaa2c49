/*
 * dvf_hip.h -- C ABI of libdvf_hip.so: the MI355X (gfx950) kernels behind the
 * depth + visual-odometry training hot path of Depth-VO-Feat (pytorch_version/).
 *
 * Conventions (every entry point):
 *   - plain C, no torch types; every pointer is a DEVICE pointer to fp32 data unless
 *     the parameter is documented as a host array;
 *   - tensors are contiguous NCHW (the reference's layout);
 *   - `stream` is a hipStream_t passed as void*; the call only enqueues work on it
 *     (no allocation, no synchronisation, capturable in a hipGraph);
 *   - workspaces are passed in by the caller; sizes come from the *_workspace_floats
 *     query functions;
 *   - the return value is 0 (DVF_OK) or a negative DVF_ERR_* code; nothing throws.
 *
 * The host side that binds these (ctypes, `depth-vo-feat_amd/dvf/lib.py`) mirrors the
 * reference's Python API one to one; the reference call site each entry replaces is
 * cited per function as pytorch_version/<file>:<line>.
 */
#ifndef DVF_HIP_H
#define DVF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVF_OK 0
#define DVF_ERR_INVALID_ARG (-1)
#define DVF_ERR_LAUNCH (-2)
#define DVF_ERR_UNSUPPORTED (-3)

/* geometry flags (bit field) */
#define DVF_ROT_QUAT 1u      /* pose[3:6] are the last 3 quaternion coefficients (inverse_warp.py:117-138); default euler (:77-114) */
#define DVF_PAD_BORDER 2u    /* padding_mode='border'; default 'zeros' incl. the coords-set-to-2 overwrite (inverse_warp.py:67-71) */
#define DVF_ALIGN_CORNERS 4u /* grid_sample(align_corners=True); default False = what the reference runs as (SURVEY.md preamble #5) */
#define DVF_POSE_SE3 8u      /* pose = (wx,wy,wz,ux,uy,uz): exponential map with t = R u (se3_generate.py:7-53, caffe/python/pygeometry.py:6-114);
                                the front end of unsupervise_dvo.py:98-100 */
#define DVF_PIXEL_COORDS 16u /* sample at pixel coordinates u = fx X/(Z+1e-12) + cx, taps bounds-checked individually, no coords
                                overwrite and no depth clamp: Caffe GeoTransform -> PinHole -> InverseWarping semantics
                                (geometry_transformation.cu:10-47, pin_hole_layer.cu:10-50, inverse_warping_layer.cu:10-52) */

#define DVF_CAFFE_ABSLOSS 32u /* photometric loss normalised and differentiated like Caffe's AbsLoss (abs_loss_layer.cu:10-34,
                                experiments/depth_odometry_feature/train.prototxt:4428-4446): sum |warped - target| / B (per-sample
                                sum, not a mean), NO exact-zero validity mask, d|d|/dd = (d > 0) - (d <= 0) */

/* activation codes for the convolution epilogues */
#define DVF_ACT_NONE 0
#define DVF_ACT_RELU 1
#define DVF_ACT_SIGMOID_AFFINE 2 /* alpha * sigmoid(x) + beta  (DispNetS.py:112; masks use alpha=1, beta=0) */

#define DVF_MAX_VIEWS 4
#define DVF_MAX_SEGS 5

int dvf_version(void);
const char *dvf_error_string(int code);
/* 1 when the library was built with -DDVF_TUNING (tuning knobs read from the environment, kernel ablation switches);
 * the product build returns 0: it reads no environment variable and cannot be switched into computing partial results. */
int dvf_build_has_tuning(void);
/* Which kernels the LAST dvf_conv2d_* call of this thread launched: up to DVF_PLAN_MAX records (further ones are dropped) of
 * DVF_PLAN_INTS ints, copied to the HOST array `out`; returns the number of ints written.  Int 0 of a record is its kernel
 * family (DVF_K_*), the others are named per family, in order, unused ones 0 (the csrc/dvf_common.h note functions write
 * them, dvf.lib.PlanRecord of the host binding reads them by these names):
 *   conv_pipe       MT, NT, WM, CK, TBU, KS, BN, NST, threads, lds, flags
 *                   flags = out_mode | ncls << 4 | x4 << 8 | blocked << 9 | lr << 10 | npi << 11   (DVF_PLAN_*_SHIFT / _MASK)
 *                   out_mode 0 fused, 1 atomic, 2 ws; ncls parity classes; x4 16-byte lanes; blocked accumulation; lr the
 *                   low-register form (two blocks a CU); npi its pieces per item
 *   conv_gather     MT, NT, WM = 1, CK, TBU = 0, KS, BN = 1, NST = 1, threads, lds, flags = out_mode | ncls << 4
 *   head_fwd        C_out, nseg
 *   head_dgrad      C_out
 *   head_wgrad      C_out, ordered   (1: per-block partials added in block order)
 *   conv_wgrad      MT, NTW, prefetch, CK, BH, PSPLIT, vec_p, stride, threads, lds, taps = KH * KW
 *   head_seg_dgrad  segc
 *   wgrad_pipe      tile = MT | TILE << 8, NTW, lanes = x4 | ordered << 1, CK, stride, pieces, blocks, lds, taps, row_stride, nseg
 *   dconvt_fwd      C_out, KH
 * The planner is shape dependent; tests use this to show that every plan of the benchmark step is parity-tested. */
enum { DVF_K_PIPE = 1, DVF_K_GATHER = 2, DVF_K_HEAD_FWD = 3, DVF_K_HEAD_DGRAD = 4, DVF_K_HEAD_WGRAD = 5, DVF_K_WGRAD = 6,
       DVF_K_HEAD_SEG_DGRAD = 7, DVF_K_WGRAD_PIPE = 8, DVF_K_DCONVT_FWD = 9 };
#define DVF_PLAN_INTS 12
#define DVF_PLAN_MAX 8
#define DVF_PLAN_MODE_MASK 15 /* conv_pipe / conv_gather flags */
#define DVF_PLAN_NCLS_SHIFT 4
#define DVF_PLAN_NCLS_MASK 15
#define DVF_PLAN_X4_SHIFT 8
#define DVF_PLAN_BLOCKED_SHIFT 9
#define DVF_PLAN_LR_SHIFT 10
#define DVF_PLAN_NPI_SHIFT 11
#define DVF_PLAN_WG_MT_MASK 255 /* wgrad_pipe tile */
#define DVF_PLAN_WG_TILE_SHIFT 8
#define DVF_PLAN_WG_X4_SHIFT 0 /* wgrad_pipe lanes */
#define DVF_PLAN_WG_ORDERED_SHIFT 1
int dvf_conv2d_last_plans(int *out, int max_ints);

/* ---------------------------------------------------------------- inverse warp (image out)
 * Replaces inverse_warp.inverse_warp (pytorch_version/inverse_warp.py:160-193; copy at
 * loss_functions.py:198-231): pixel2cam -> pose_vec2mat -> K@[R|t] -> cam2pixel -> grid_sample.
 *   img [B,C,H,W], depth [B,H,W], pose [B,6] (tx,ty,tz,rx,ry,rz), K/Kinv [B,3,3] -> out [B,C,H,W]. */
int dvf_inverse_warp_fwd(const float *img, const float *depth, const float *pose, const float *K,
                         const float *Kinv, float *out, int B, int C, int H, int W, uint32_t flags,
                         void *stream);
/* Backward of the above for an incoming grad_out [B,C,H,W].  Any of g_img / g_depth / g_pose may be
 * NULL (not needed).  g_img must be ZEROED by the caller (scatter-add target).  pose_ws: >=
 * dvf_pose_ws_floats(1, B) floats, zeroed by this call. */
int dvf_inverse_warp_bwd(const float *img, const float *depth, const float *pose, const float *K,
                         const float *Kinv, const float *grad_out, float *g_img, float *g_depth,
                         float *g_pose, float *pose_ws, int B, int C, int H, int W, uint32_t flags,
                         void *stream);
int64_t dvf_pose_ws_floats(int V, int B);
/* The same backward with the pose gradient summed in a FIXED order (deterministic mode): every block stores its [R|t]
 * partial and one pass adds them in block order, instead of float atomics in order of arrival -- g_pose is then
 * bit-reproducible from run to run like g_depth (g_img stays a scatter-add).  ws: >= dvf_inverse_warp_ordered_ws_floats(B, H, W)
 * floats, contents irrelevant, nothing needs zeroing.  Build-side addition: the reference's autograd has no such choice. */
int64_t dvf_inverse_warp_ordered_ws_floats(int B, int H, int W);
int dvf_inverse_warp_bwd_ordered(const float *img, const float *depth, const float *pose, const float *K,
                                 const float *Kinv, const float *grad_out, float *g_img, float *g_depth,
                                 float *g_pose, float *ws, int B, int C, int H, int W, uint32_t flags,
                                 void *stream);

/* ---------------------------------------------------------------- stand-alone geometry helpers
 * The public building blocks of inverse_warp.py, for callers that use them directly (the fused kernels above do
 * not go through these).
 *   pose_vec2mat (inverse_warp.py:141-157; euler2mat :77-114, quat2mat :117-138): pose [n,6] -> [n,3,4];
 *     backward: g_mat [n,3,4] -> g_pose [n,6], ws = n*12 floats.
 *   pixel2cam (:26-40): depth [B,H,W], Kinv [B,3,3] -> cam [B,3,H,W]; backward -> g_depth.
 *   cam2pixel (:43-74): cam [B,3,H,W], rot [B,3,3] or NULL, tr [B,3] or NULL -> grid [B,H,W,2] (x_n, y_n);
 *     backward: g_cam [B,3,H,W] (may be NULL) and g_rot_tr_ws [B,12] = (g_tr[3], g_rot[9]) (may be NULL). */
int dvf_pose_vec2mat_fwd(const float *pose, float *out, int n, uint32_t flags, void *stream);
int dvf_pose_vec2mat_bwd(const float *pose, const float *g_mat, float *g_pose, float *ws, int n, uint32_t flags,
                         void *stream);
int dvf_pixel2cam_fwd(const float *depth, const float *Kinv, float *cam, int B, int H, int W, void *stream);
int dvf_pixel2cam_bwd(const float *Kinv, const float *g_cam, float *g_depth, int B, int H, int W, void *stream);
int dvf_cam2pixel_fwd(const float *cam, const float *rot, const float *tr, float *grid, int B, int H, int W,
                      uint32_t flags, void *stream);
int dvf_cam2pixel_bwd(const float *cam, const float *rot, const float *tr, const float *g_grid, float *g_cam,
                      float *g_rot_tr_ws, int B, int H, int W, uint32_t flags, void *stream);

/* ---------------------------------------------------------------- fused warp + photometric L1
 * Replaces the body of loss_functions.photometric_reconstruction_loss (loss_functions.py:7-20) and of
 * one_scale() in loss_functions_sfm.photometric_reconstruction_loss (loss_functions_sfm.py:10-36):
 * for every view v: warp src_v with pose_v, exact-zero mask, optional explainability mask, |.|, mean
 * over B*C*H*W; the views are summed.  One kernel per pyramid scale handles all V views of a pixel; the 2x2
 * source neighbourhoods of a 64x4 target tile are staged through an LDS footprint tile.
 *   tgt [B,C,H,W]; srcs: HOST array of V device pointers, each [B,C,H,W]; depth [B,H,W];
 *   pose [V,B,6]; K/Kinv [B,3,3]; mask NULL or [B,V,H,W];
 *   in_scale: every tgt / src value is used as fl(in_scale * x) -- the `0.004 * img` of unsupervise.py:101 without
 *     materialising scaled copies (1.0f = the reference signature; must not be 0);
 *   loss_out: 1 float (sum over views), view_loss: NULL or V floats;
 *   partials: workspace >= dvf_photo_partials_floats(B,H,W,V) floats. */
int dvf_photo_loss_fwd(const float *tgt, const float *const *srcs, int V, const float *depth,
                       const float *pose, const float *K, const float *Kinv, const float *mask,
                       float *loss_out, float *view_loss, float *partials, int B, int C, int H, int W,
                       float in_scale, uint32_t flags, void *stream);
int64_t dvf_photo_partials_floats(int B, int H, int W, int V);
/* Backward: grad_loss is a DEVICE scalar (upstream gradient).  Outputs (each may be NULL):
 *   g_depth [B,H,W] (written), g_pose [V,B,6] (written), g_tgt [B,C,H,W] (written),
 *   g_srcs: HOST array of V device pointers or NULL entries, each [B,C,H,W], ZEROED by the caller
 *   (scatter-add target: accumulated per block in LDS, flushed with row-contiguous atomics),
 *   g_mask [B,V,H,W] (written).  pose_ws >= dvf_photo_pose_ws_floats(B,H,W,V) floats (per-block [R|t] partials,
 *   summed in fixed order: the pose gradient is bit-reproducible).  g_tgt / g_srcs need C <= 32
 *   (DVF_ERR_UNSUPPORTED otherwise; the reference's feature maps have 32 channels, feat_extractor.py:13-36). */
int dvf_photo_loss_bwd(const float *tgt, const float *const *srcs, int V, const float *depth,
                       const float *pose, const float *K, const float *Kinv, const float *mask,
                       const float *grad_loss, float *g_depth, float *g_pose, float *g_tgt,
                       float *const *g_srcs, float *g_mask, float *pose_ws, int B, int C, int H, int W,
                       float in_scale, uint32_t flags, void *stream);
int64_t dvf_photo_pose_ws_floats(int B, int H, int W, int V);

/* ---------------------------------------------------------------- input pipeline: frame -> network input on the GPU
 * Replaces, per frame, `imresize(imread(f).astype(np.float32), (H, W))` of the reference's loaders (un_dataset.py:63-66,
 * dataset.py:50-51; scipy.misc.imresize = bytescale [min,max]->[0,255] + PIL BILINEAR on uint8), bit for bit:
 *   src_hwc uint8 [IH,IW,C] (the decoded frame) -> dst_chw float32 [C,OH,OW] (integer values 0..255).
 * hbounds/hcoef [OW,2]/[OW,hksize] and vbounds/vcoef [OH,2]/[OH,vksize]: DEVICE int32 tables of PIL's separable triangle
 * filter in 22-bit fixed point (dvf/image_ops.py builds them as Pillow's precompute_coeffs / normalize_coeffs_8bpc do);
 * tmp: uint8 [IH,OW,C] workspace; minmax: 2 int32 workspace. */
int dvf_imresize_u8(const uint8_t *src_hwc, int IH, int IW, int C, const int *hbounds, const int *hcoef, int hksize,
                    const int *vbounds, const int *vcoef, int vksize, uint8_t *tmp, int *minmax, float *dst_chw, int OH, int OW,
                    void *stream);

/* ---------------------------------------------------------------- training augmentation (build-side extension, opt-in)
 * Random horizontal flip, zoom-and-crop and colour perturbation on the device, in place of the host transforms of
 * pytorch_version/custom_transforms.py:46-84 (wired in train.py:89-101).  tests/augment_ref.py is the definition; parity is
 * unpinned (the reference's transforms no longer import) and departs from them in two documented places (below).
 * params [B,12], one record per sample, applied to every frame of the sample:
 *   {flip 0|1, sw, sh, ox, oy, colour_on 0|1, gamma, brightness, gain_r, gain_g, gain_b, 0}: the frame is zoomed to sw x sh
 *   (integers >= W, H), cropped at the integer offset (ox, oy), then mirrored.  The caller validates the records
 *   (dvf/augment.py::validate_params); tap indices are clamped, so no record makes the kernel read outside a frame.
 * dvf_augment_frames: src / dst are HOST arrays of F device pointers (1 <= F <= 8), each [B,3,H,W]; one launch for all frames.
 *   For output (y, x): xc = flip ? W-1-x : x; u = (xc + ox + 0.5) W/sw - 0.5, v = (y + oy + 0.5) H/sh - 0.5, clamped to the
 *   frame; bilinear taps x0 = floor(u), x1 = min(x0+1, W-1) (likewise y).  sw = W, ox = 0 gives a bit-exact copy / mirror.
 *   Colour (only where colour_on; otherwise bits pass through): n = value/value_max; n = n^gamma, evaluated as
 *   exp2(gamma log2 n); value = value_max clamp(n brightness gain_c, 0, 1).
 *   The gather reads the whole source: a dst that overlaps any src or another dst is DVF_ERR_INVALID_ARG, as is C != 3.
 * dvf_augment_geometry: K' = A K M, Kinv' = M Kinv A^-1 [B,3,3] with sx = sw/W, sy = sh/H, cxo = (sx-1)/2 - ox, cyo likewise,
 *   A = [[sx,0,cxo],[0,sy,cyo],[0,0,1]], M = I, or under flip A = [[-sx,0,W-1-cxo],[0,sy,cyo],[0,0,1]], M = diag(-1,1,1) --
 *   the exact map of pixel indices in the warp's convention (integer index = pixel centre, inverse_warp.py:8-15); the
 *   reference scales by the untruncated factor without the half-pixel term (custom_transforms.py:73-74,81-82) and mirrors
 *   cx as w - cx (:55).  Under flip T_tr [B,6] (t, r) is multiplied by (-1,1,1,1,-1,-1) and T_se3 [B,6] (w, u) by
 *   (1,-1,-1,-1,1,1).  Every output may alias its input. */
int dvf_augment_frames(const float *const *src, float *const *dst, int F, const float *params, int B, int C, int H, int W,
                       float value_max, void *stream);
int dvf_augment_geometry(const float *params, const float *K, const float *Kinv, const float *T_tr, const float *T_se3,
                         float *K_out, float *Kinv_out, float *T_tr_out, float *T_se3_out, int B, int W, int H, void *stream);

/* ---------------------------------------------------------------- edge-aware smoothness (paper / Caffe graph variant)
 * experiments/depth_odometry_feature/train.prototxt:4452-4661 with caffe/include/caffe/filler.hpp:267-316 and
 * abs_loss_layer.cu:10-34: loss_out[0] (+)= weight * (sum |exp(-k sum_c |d_y I_c|) d_y D| + sum |exp(-k sum_c |d_x I_c|) d_x D|) / B
 * over the (H-2) x (W-2) interior (3x3 valid central differences, +-0.5), I = in_scale * img [B,C,H,W], D = inv_depth [B,H,W];
 * backward writes g_inv_depth [B,H,W] (AbsLoss sign convention: zero counts as positive).  Parity unpinned (no Caffe here). */
int dvf_edge_smooth_fwd(const float *inv_depth, const float *img, float *loss_out, float *partials, int B, int C, int H, int W,
                        float in_scale, float edge_k, float weight, int accumulate, void *stream);
int64_t dvf_edge_smooth_partials_floats(int B, int H, int W);
int dvf_edge_smooth_bwd(const float *inv_depth, const float *img, const float *grad_loss, float *g_inv_depth, int B, int C, int H,
                        int W, float in_scale, float edge_k, float weight, void *stream);

/* ---------------------------------------------------------------- SSIM + L1 appearance term (build-side extension, opt-in)
 * The reference has no SSIM (SURVEY.md preamble #1): there is NO reference call site.  The term plugs in where
 * pytorch_version/loss_functions_sfm.py:23-35 / loss_functions.py:12-19 form `diff`, on an already warped reference
 * (dvf_inverse_warp_fwd).  Definition (monodepth2 form), x = fl(in_scale * tgt), y = fl(in_scale * warped), both [B,C,H,W]:
 *   per pixel and channel a 3x3 window, uniform weights 1/9, REFLECTION border (index -1 -> 1, H -> H-2, same for W):
 *     mx, my, vx = mean((x - mx)^2), vy = mean((y - my)^2), cxy = mean((x - mx)(y - my))         (centred form)
 *   SSIM  = ((2 mx my + c1)(2 cxy + c2)) / ((mx^2 + my^2 + c1)(vx + vy + c2))
 *   dssim = clamp((1 - SSIM) / 2, 0, 1), derivative 0 outside the clamp range
 *   term  = alpha * dssim + (1 - alpha) * |x - y|
 *   valid = 1 - prod_c [y_c == 0] at the centre pixel (the reference's exact-zero mask), no gradient
 *   loss_out[0] (+)= sum(term * valid * m) / (B C H W)   (masked pixels stay in the denominator; accumulate != 0 adds)
 * mask: NULL or the explainability mask of this view, element (b, y, x) at mask[b * mask_batch_stride + y * W + x]
 *   (view v of a [B,V,H,W] tensor: pointer + v*H*W, stride V*H*W -- no copy); it receives a gradient.
 * partials: workspace >= dvf_ssim_partials_floats(B,H,W) floats; the loss is summed in a fixed order (bit-reproducible).
 * Backward (gather form, no atomics): grad_loss is a DEVICE scalar; g_warped / g_tgt [B,C,H,W] and g_mask (addressed like
 *   mask, same batch stride; = sum_c term * valid * grad_loss / (B C H W)) may each be NULL; every element of a given
 *   output is written exactly once, nothing needs zeroing.
 * DVF_ERR_INVALID_ARG for H or W < 3, C*H*W >= 2^31, B > 65535.  Parity unpinned (nothing in the reference to compare with). */
int64_t dvf_ssim_partials_floats(int B, int H, int W);
int dvf_ssim_loss_fwd(const float *tgt, const float *warped, const float *mask, int64_t mask_batch_stride, float *loss_out,
                      float *partials, int B, int C, int H, int W, float in_scale, float alpha, float c1, float c2, int accumulate,
                      void *stream);
int dvf_ssim_loss_bwd(const float *tgt, const float *warped, const float *mask, int64_t mask_batch_stride, const float *grad_loss,
                      float *g_warped, float *g_tgt, float *g_mask, int B, int C, int H, int W, float in_scale, float alpha,
                      float c1, float c2, void *stream);

/* ---------------------------------------------------------------- per-pixel minimum reprojection + auto-mask (extension, opt-in)
 * The second part of the monodepth2 appearance term; like SSIM there is NO reference call site, parity is unpinned and
 * tests/minreproj_ref.py is the definition.  x = fl(in_scale * tgt) [B,C,H,W]; cands: HOST array of K device pointers to
 * [B,C,H,W] images, used as y_k = fl(in_scale * cands[k]): the V warped references (outputs of dvf_inverse_warp_fwd),
 * 1 <= V <= 4, then -- auto_mask != 0 -- the V unwarped references in the same order (K = V or 2V).  Per pixel p:
 *   e_k(p) = (1/C) sum_c [alpha * dssim_c(x, y_k)(p) + (1 - alpha) * |x_c(p) - y_k,c(p)|]     (dssim as above; alpha = 0 allowed)
 *   usable : a warped candidate unless it is exactly zero in all channels at p (no gradient); an identity candidate always
 *   k*(p)  = the LOWEST index among the usable candidates that attain min_k e_k(p): a tie goes to a warped view before an
 *            identity one, there is no tie-break noise; "none" when no candidate is usable
 *   loss_out[0] (+)= sum_p e_k*(p)(p) / (B H W)   (pixels with no usable candidate add 0 and stay in the denominator; the
 *            value of a winning identity candidate is included, it is constant with respect to the networks)
 * select: uint8 [B,H,W], k*(p), 255 = none.  counts: K+1 int32, the number of pixels per selection, the last one "none".
 * partials: workspace >= dvf_minreproj_partials_floats(B,H,W,K) floats.  Loss and counts are reduced from per-block
 *   partials in a fixed order, without atomics: both are bit-reproducible.
 * Backward (one launch, gather form, no atomics): the selection is piecewise constant; g_warped[k] (HOST array of V device
 *   pointers, the array or any entry may be NULL) collects the windows q with k*(q) = k, g_tgt (may be NULL) the selected
 *   candidate of every window, identity candidates included; identity sources get no gradient.  grad_loss is a DEVICE
 *   scalar; every element of a given output is written exactly once, nothing needs zeroing.  The clamp gate of dssim
 *   behaves as in dvf_ssim_loss_bwd.
 * DVF_ERR_INVALID_ARG for null pointers, V outside 1..4, H or W < 3, C*H*W >= 2^31, B > 65535.  No allocation, no
 * synchronisation: the calls can be captured in a HIP graph. */
int64_t dvf_minreproj_partials_floats(int B, int H, int W, int K);
int dvf_minreproj_fwd(const float *tgt, const float *const *cands, int V, int auto_mask, float *loss_out, uint8_t *select,
                      int32_t *counts, float *partials, int B, int C, int H, int W, float in_scale, float alpha, float c1, float c2,
                      int accumulate, void *stream);
int dvf_minreproj_bwd(const float *tgt, const float *const *cands, int V, int auto_mask, const uint8_t *select,
                      const float *grad_loss, float *g_tgt, float *const *g_warped, int B, int C, int H, int W, float in_scale,
                      float alpha, float c1, float c2, void *stream);

/* ---------------------------------------------------------------- edge-aware smoothness of the mean-normalised disparity
 * (extension, opt-in).  The regulariser of the monodepth2 recipe; the reference's smoothness terms are the second-order one
 * below and the Caffe graph's un-normalised one above, so there is NO reference call site, parity is unpinned and
 * tests/normsmooth_ref.py is the definition.  disp [B,1,H,W], I = fl(in_scale * img) with img [B,C,H,W]; per image b:
 *   m_b  = mean over (H,W) of disp_b                      n = disp / (m_b + eps)
 *   wx   = exp(-mean_c |I(y,x) - I(y,x+1)|)               wy = exp(-mean_c |I(y,x) - I(y+1,x)|)
 *   loss_out[0] (+)= weight * (mean(wx |n(y,x) - n(y,x+1)|) + mean(wy |n(y,x) - n(y+1,x)|))       (accumulate != 0 adds)
 *   the two means over B*H*(W-1) and B*(H-1)*W elements; only disp receives a gradient; d|v|/dv = 0 at v = 0.
 * With the mean fixed the term is linear in |delta disp|, so the forward is ONE tile pass over disp and img that leaves three
 *   sums per block (sum disp, Sx = sum wx |dx disp|, Sy = sum wy |dy disp|) in `partials` (>= dvf_norm_smooth_partials_floats(B,H,W)
 *   floats) plus one small finishing launch: stats [B,2] = (m_b + eps, T_b), T_b = Sx_b / (B H (W-1)) + Sy_b / (B (H-1) W),
 *   loss = weight * sum_b T_b / |m_b + eps|.  Every sum is taken in a fixed order, without atomics: bit-reproducible.
 * Backward (one launch, gather form, no atomics): stats is the forward's output, grad_loss a DEVICE scalar; every pixel collects
 *   sign(delta) * w from its up to four neighbours (weights recomputed from the image) into A_p, which carries the two 1/count
 *   factors, and writes g_disp [B,1,H,W] = grad_loss * weight * (A_p / (m_b + eps) - T_b / ((m_b + eps)^2 H W)) (for a negative
 *   mean the first denominator is |m_b + eps| and the second keeps its sign).  Every element is written exactly once, nothing
 *   needs zeroing.
 * Checked on the host before anything is launched: DVF_ERR_INVALID_ARG for a null pointer, B <= 0, C <= 0, H < 2 or W < 2 (a mean
 *   over W-1 or H-1 elements would be empty), B > 65535, C*H*W >= 2^31.  No allocation, no synchronisation: capturable. */
int64_t dvf_norm_smooth_partials_floats(int B, int H, int W);
int dvf_norm_smooth_fwd(const float *disp, const float *img, float *loss_out, float *stats, float *partials, int B, int C, int H,
                        int W, float in_scale, float eps, float weight, int accumulate, void *stream);
int dvf_norm_smooth_bwd(const float *disp, const float *img, const float *stats, const float *grad_loss, float *g_disp, int B,
                        int C, int H, int W, float in_scale, float eps, float weight, void *stream);

/* ---------------------------------------------------------------- smoothness loss
 * Replaces one map of smooth_loss (loss_functions.py:23-41 ; loss_functions_sfm.py:59-77):
 * weight * (mean|dx2| + mean|dxdy| + mean|dydx| + mean|dy2|) of a [N,H,W] stack of planes (N = B*C).
 * loss_out[0] (+)= result: accumulate != 0 adds to the value already there (multi-scale lists). */
int dvf_smooth_loss_fwd(const float *map, float *loss_out, float *partials, int N, int H, int W,
                        float weight, int accumulate, void *stream);
int64_t dvf_smooth_partials_floats(int N, int H, int W);
int dvf_smooth_loss_bwd(const float *map, const float *grad_loss, float *g_map, int N, int H, int W,
                        float weight, void *stream);

/* ---------------------------------------------------------------- convolutions (fp32 MFMA)
 * One descriptor for nn.Conv2d and nn.ConvTranspose2d as the reference's networks use them
 * (DispNetS.py:7-34, PoseExpNet_sfm.py:6-17, feat_extractor.py:6-41): square-ish kernels up to 7x7,
 * stride 1 or 2, symmetric padding, groups = 1.  H_out/W_out are the sizes actually kept, i.e. AFTER
 * crop_like (DispNetS.py:37-39): the kernels never compute cropped-away pixels.
 * Weight layouts are torch's: Conv2d [C_out,C_in,KH,KW]; ConvTranspose2d [C_in,C_out,KH,KW].
 * The input may be a VIRTUAL CONCAT of up to DVF_MAX_SEGS tensors [N,seg_channels[i],H_in,W_in]
 * (replaces torch.cat at DispNetS.py:98-128): in_segs / din_segs are HOST arrays of device pointers. */
typedef struct dvf_conv_desc {
    int N, C_in, H_in, W_in, C_out, H_out, W_out, KH, KW, stride, pad, transposed;
    int act;           /* DVF_ACT_*: fused epilogue of the forward */
    float alpha, beta; /* DVF_ACT_SIGMOID_AFFINE parameters */
} dvf_conv_desc;

/* out = act(conv(cat(in_segs), w) + bias).  Replaces nn.Conv2d / nn.ConvTranspose2d (+ReLU / Sigmoid, and the
 * alpha*sigmoid+beta of DispNetS.py:112) forward.  bias may be NULL; w may not.  packed (may be NULL): the op_kind 0
 * copy of w (below).  The pipelined kernel reads it when its plan accepts the call; otherwise -- refused for the geometry,
 * or at run time for an operand of a 16-byte-lane plan that is not 16-byte aligned -- the unpacked kernels read w. */
int dvf_conv2d_fwd(const dvf_conv_desc *d, const float *const *in_segs, const int *seg_channels, int nseg,
                   const float *packed, const float *w, const float *bias, float *out, float *ws, int64_t ws_floats,
                   void *stream);
/* d(loss)/d(input segment i) for i with din_segs[i] != NULL, given dpre = d(loss)/d(pre-activation output).  packed (may be
 * NULL): the op_kind 1 copy of w; input segments it has no share of (at most 32 channels) and segments whose plan is refused
 * at run time are computed from w.  mask_segs (may be NULL, and so may its entries): mask_segs[s] != NULL says input segment
 * s is the output y of a ReLU convolution (reference: nn.ReLU(inplace=True) after every conv, DispNetS.py:10-16,30-41,
 * PoseExpNet_sfm.py:9-13): din_segs[s] leaves as (y > 0) ? din : 0 -- which is dL/dpre of that layer when every consumer
 * of y does the same (the ReLU mask distributes over the sum autograd forms).  Replaces torch's ThresholdBackward. */
int dvf_conv2d_dgrad(const dvf_conv_desc *d, const float *dpre, const float *packed, const float *w, float *const *din_segs,
                     const int *seg_channels, int nseg, float *ws, int64_t ws_floats, const float *const *mask_segs,
                     void *stream);
/* d(loss)/d(w) in w's own layout; accumulate != 0 adds to dw, otherwise dw is zeroed first.  dbias (may be NULL): the bias
 * gradient of the same layer, dbias[c] (+)= sum over (n, y, x) of dpre[n][c][y][x] (torch: the bias output of
 * ConvolutionBackward).  For Conv2d layers the pipelined weight-gradient kernel multiplies its dpre tile by one more
 * column -- of ones -- so no extra pass reads dpre; otherwise one reduction pass runs after it.
 * ws (may be NULL): with dvf_conv2d_wgrad_ws_floats(...) floats both gradients are run-to-run DETERMINISTIC -- the
 * reference's CPU path is (torch CPU ConvolutionBackward, train.py:213): the pipelined kernel splits the pixel reduction over
 * all CUs, every block stores its partial tiles and one pass adds them in block order, instead of float atomics in order
 * of arrival (ws == NULL or too small). */
int64_t dvf_conv2d_wgrad_ws_floats(const dvf_conv_desc *d, const int *seg_channels, int nseg);
int dvf_conv2d_wgrad(const dvf_conv_desc *d, const float *const *in_segs, const int *seg_channels, int nseg,
                     const float *dpre, float *dw, int accumulate, float *dbias, int accumulate_dbias, float *ws,
                     int64_t ws_floats, void *stream);

/* Packed weights for the LDS-DMA pipelined kernel: the exact LDS image of every reduction chunk.  op_kind 0 = forward,
 * 1 = dgrad.  Protocol: n = dvf_conv2d_packed_floats(...) (negative = DVF_ERR_*; DVF_ERR_UNSUPPORTED means "no packed copy
 * for this geometry": pass packed = NULL); the caller allocates n floats and ZERO-FILLS them once; dvf_conv2d_pack()
 * refreshes the copy whenever w changed (after every optimizer step, train.py:214).  The packing depends on the whole
 * descriptor (incl. N, H, W) and on seg_channels: use the same ones everywhere. */
int64_t dvf_conv2d_packed_floats(const dvf_conv_desc *d, const int *seg_channels, int nseg, int op_kind);
int dvf_conv2d_pack(const dvf_conv_desc *d, const int *seg_channels, int nseg, int op_kind, const float *w, float *packed,
                    void *stream);
/* Optional split-K workspace of dvf_conv2d_fwd (op_kind 0) and dvf_conv2d_dgrad (1): with ws (>= dvf_conv2d_ws_floats(...)
 * floats, contents irrelevant) small grids split the reduction over blocks that store plain partial tiles which one pass
 * sums in a fixed order (+bias, activation) -- activations are then bit-reproducible from run to run; with ws == NULL they
 * accumulate with float atomics into a zeroed output instead. */
int64_t dvf_conv2d_ws_floats(const dvf_conv_desc *d, const int *seg_channels, int nseg, int op_kind);
/* Batched packing (one launch per optimizer step instead of one per convolution): dvf_conv2d_pack_jobs() writes the
 * job records of one convolution (1 for op_kind 0, nseg for op_kind 1; DVF_PACK_JOB_BYTES each, opaque) into HOST
 * memory and their block counts into blocks_out, returning the number of jobs (or a negative DVF_ERR_*).  The caller
 * concatenates the records of all convolutions, uploads them and the exclusive prefix sum of the block counts
 * (njobs + 1 ints) to the device once, and calls dvf_conv2d_pack_batch() after every optimizer step with lds_bytes = the
 * maximum that the pack_jobs calls left in *lds_bytes_out (they only ever raise it).  block_job_dev (optional, may be
 * NULL): total_blocks ints, the job index of every block -- saves each block a binary search through the prefix. */
#define DVF_PACK_JOB_BYTES 512
int dvf_conv2d_pack_jobs(const dvf_conv_desc *d, const int *seg_channels, int nseg, int op_kind, const float *w, float *packed,
                         void *jobs_host, int max_jobs, int *blocks_out, int *lds_bytes_out);
int dvf_conv2d_pack_batch(const void *jobs_dev, const int *block_prefix_dev, const int *block_job_dev, int njobs,
                          int total_blocks, int lds_bytes, void *stream);
/* Backward of the fused activation and of the bias in one pass: dpre = dy * act'(y) (y = the forward's
 * output, [N,C,HW]); dbias[c] (+)= sum dpre (accumulate_dbias != 0 adds to dbias, otherwise it is zeroed first: a bias
 * gradient that lives in a zeroed gradient arena needs neither a memset nor a separate add).  dpre or dbias may be NULL.
 * ws (may be NULL): with dvf_act_bwd_ws_floats(N, C, HW) floats the bias gradient is run-to-run deterministic -- per-block
 * partial sums go through ws and are added in index order instead of float atomics on dbias[c]. */
int64_t dvf_act_bwd_ws_floats(int N, int C, int HW);
int dvf_act_bwd(const float *dy, const float *y, float *dpre, float *dbias, int N, int C, int HW, int act, float alpha,
                float beta, int accumulate_dbias, float *ws, int64_t ws_floats, void *stream);

/* ---------------------------------------------------------------- memory-bound helpers
 * planes = N*C throughout. */
/* F.interpolate(mode='bilinear', align_corners=False): out[Y][X] for Y<OH, X<OW with source scale
 * scale_h = H/(full OH) (0.5 for x2 up, DispNetS.py:115,121,127 -- OH/OW may be the crop_like-cropped size;
 * 2.0 for the x0.5 image pyramid of feat_extractor.py:44-46). */
int dvf_resize_bilinear_fwd(const float *in, float *out, int planes, int H, int W, int OH, int OW, float scale_h,
                            float scale_w, void *stream);
/* backward of the x2 case (gather form, no atomics): gout [planes,OH,OW] -> gin [planes,H,W] */
int dvf_upsample2x_bwd(const float *gout, float *gin, int planes, int H, int W, int OH, int OW, void *stream);
/* Integer-factor bilinear upsampling to the input resolution, optionally fused with the disparity -> depth reciprocal:
 * the full-resolution multi-scale mode of the photometric losses.  Build-side EXTENSION: the reference has no such mode and
 * there is no reference call site; parity is unpinned and tests/fullres_ref.py is the definition.
 *   in [planes,H,W] -> out [planes,factor*H,factor*W] = F.interpolate(in, (factor*H, factor*W), mode='bilinear',
 *   align_corners=False): src = (dst + 0.5) / factor - 0.5 clamped at 0, the upper tap clamped to the last row / column;
 *   recip != 0: out = 1 / (that + eps) in the same pass (the upsampled disparity is never stored).  factor is 2, 4 or 8.
 * Backward: the exact transpose, gin [planes,H,W] from gout [planes,factor*H,factor*W]; with recip != 0 gout is first
 *   multiplied by -out^2, `out` being the forward's output (NULL allowed when recip == 0).  Gather form, separable (a row
 *   pass into LDS, then a column pass), every sum in a fixed order and no atomics: bit-reproducible; gin is written once.
 * Checked on the host before anything is launched: DVF_ERR_INVALID_ARG for a null pointer, a non-positive size or
 *   planes * factor*H * factor*W >= 2^31 (the kernels index fine pixels in 32 bits); DVF_ERR_UNSUPPORTED for another factor. */
int dvf_upsample_int_fwd(const float *in, float *out, int planes, int H, int W, int factor, int recip, float eps,
                         void *stream);
int dvf_upsample_int_bwd(const float *gout, const float *out, float *gin, int planes, int H, int W, int factor, int recip,
                         void *stream);
/* y = 1 / (x + eps)  (train.py:188 eps=0; unsupervise.py:99 eps=1e-4) and its backward gx = -gy * y^2 */
int dvf_recip_fwd(const float *x, float *y, float eps, int64_t n, void *stream);
int dvf_recip_bwd(const float *gy, const float *y, float *gx, int64_t n, void *stream);
/* out[plane] = scale * mean(in[plane])  (PoseExpNet_sfm.py:72-73: mean(3).mean(2) * 0.01) */
int dvf_spatial_mean_fwd(const float *in, float *out, int planes, int HW, float scale, void *stream);
int dvf_spatial_mean_bwd(const float *gout, float *gin, int planes, int HW, float scale, void *stream);
/* F.interpolate(mode='area') = adaptive average pooling (loss_functions_sfm.py:18-19) */
int dvf_area_downsample(const float *in, float *out, int planes, int H, int W, int OH, int OW, void *stream);
/* Depthwise nn.ConvTranspose2d(C, C, kernel_size=4, stride=2, padding=1, groups=C) of FeatExtractor's top-down path
 * (feat_extractor.py:38-41) with the residual add of :72-82 fused: out = skip + convT(x) + bias.  w [C,1,4,4];
 * x [N,C,H,W]; skip/out [N,C,2H,2W]; skip, bias may be NULL.  Backward: dx, dw (+db) from dy (d skip = dy). */
int dvf_dwconvt4x4s2_fwd(const float *x, const float *w, const float *bias, const float *skip, float *out, int N, int C,
                         int H, int W, void *stream);
int dvf_dwconvt4x4s2_bwd(const float *x, const float *w, const float *dy, float *dx, float *dw, float *db, int N, int C,
                         int H, int W, void *stream);
/* explainability_loss of one scale (loss_functions_sfm.py:49-56): loss_out[0] (+)= -mean(max(log mask, -100));
 * partials: workspace of >= 1024 floats.  Backward: g_mask = -grad_loss / (n * mask). */
int dvf_bce_ones_fwd(const float *mask, float *loss_out, float *partials, int64_t n, int accumulate, void *stream);
int dvf_bce_ones_bwd(const float *mask, const float *grad_loss, float *g_mask, int64_t n, void *stream);
/* torch.optim.Adam step (train.py:154-156, unsupervise.py:241) over a flat arena of n floats.
 * opt_state: DEVICE float[4] = {step, lr, step_size, bc2_sqrt}; the caller initialises {0, lr, 0, 0}.
 * advance_step != 0 increments step and refreshes the derived entries first (once per optimizer step).
 * grad_scale multiplies the gradient (1/world_size after a sum all-reduce). */
int dvf_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float *opt_state,
                  int advance_step, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                  void *stream);

/* ---------------------------------------------------------------- depth validation against ground truth
 * Per-image masked depth error metrics with exact median scaling: the reference's compute_errors
 * (loss_functions_sfm.py:80-116) plus the rmse / rmse_log columns of the Eigen protocol, as a few launches and no host
 * synchronisation.  gt, pred [B,H,W] fp32 at the same size; out [B][12].  Per image:
 *   valid = gt > gt_lo && gt < gt_hi && y1 <= y < y2 && x1 <= x < x2   (strict in gt: a NaN gt is invalid; the Garg crop of
 *           :92-93 is the rectangle, an empty rectangle is legal)
 *   p     = clamp(pred, clamp_lo, clamp_hi)                             (a NaN prediction stays NaN)
 *   DVF_DM_MEDIAN_SCALE: s = fl(med(gt_valid) / med(p_valid)), p = fl(p * s); med = the LOWER median, the element of rank
 *           (n-1)/2 (what torch.median returns), found exactly by a three-pass radix select on the bit patterns
 *   DVF_DM_RECLAMP: p is clamped again after scaling (depth_eval.evaluate)
 *   out row = [abs_diff, abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, n_valid, med_gt, med_pred, n_nan], means over the valid
 *           pixels, a_e = share with max(g/p, p/g) < 1.25^e, medians before scaling, n_nan = valid pixels whose prediction
 *           is NaN: with n_nan > 0 the eight metrics (and med_pred) are NaN; with n_valid == 0 the row is all zeros.
 * ws: dvf_depth_metrics_ws_floats(B, H, W) floats, zeroed by the call itself.  Integer atomics and per-block partials added in
 * a fixed order only: two runs are bit-identical.  No allocation, no synchronisation: graph-capturable.
 * Checked on the host before anything is launched: DVF_ERR_INVALID_ARG for a null pointer, a non-positive size, ws_floats
 * below the query, a rectangle outside [0,H] x [0,W] (or y1 > y2, x1 > x2), clamp_lo <= 0, clamp_lo > clamp_hi, gt_lo < 0,
 * B * H * W >= 2^31 or B > 65535. */
#define DVF_DM_MEDIAN_SCALE 1u
#define DVF_DM_RECLAMP 2u
int64_t dvf_depth_metrics_ws_floats(int B, int H, int W);
int dvf_depth_metrics(const float *gt, const float *pred, float *out /* [B][12] */, float *ws, int64_t ws_floats, int B, int H,
                      int W, int y1, int y2, int x1, int x2, float gt_lo, float gt_hi, float clamp_lo, float clamp_hi,
                      uint32_t flags, void *stream);

/* ---------------------------------------------------------------- depth ground truth from LiDAR sweeps
 * The sparse depth maps that the Eigen protocol scores against: the reference's generate_depth_map
 * (tools/eval_depth_utils.py:172-224) for B frames in one call.  points [total][4] fp32 = the raw velodyne quadruples
 * (forward, left, up, reflectance) of all frames back to back, 16-byte aligned; offsets [B+1] DEVICE ints: frame b owns points
 * offsets[b] .. offsets[b+1]-1; proj [B][3][4] DEVICE DOUBLES = P_rect_0c * R_rect_00 * Tr_velo_to_cam; depth [B][H][W] fp32 out.
 * Per frame b and per point (x, y, z, .) of it (the fourth component is ignored and taken as 1):
 *   kept only if x >= 0                                               (a NaN x is dropped)
 *   p = proj[b] * (x, y, z, 1) in fp64, the floats converted exactly
 *   u = rint(p0 / p2) - 1, v = rint(p1 / p2) - 1                      (half to even, as np.round; the -1 is KITTI's MATLAB
 *                                                                      convention, kept by the reference)
 *   kept only if u >= 0 && v >= 0 && u < W && v < H                   (NaN and +-inf coordinates, p2 == 0, fail)
 *   d = (float)p2, or with DVF_VD_VELODYNE_DEPTH d = x                (the reference's vel_depth=True)
 *   depth[b][v][u] = max(0, min over the kept points that land there of d); a pixel that no point reaches is 0.
 * The minimum comes first and the clamp second (:216-217): one point of negative camera depth on a pixel makes it "no
 * measurement".  One departure from the reference: it finds collisions through the key row * (W - 1) + col - 1, which pixel
 * (r, W-1) shares with pixel (r+1, 0), so one of those two can receive the minimum over both; this entry takes the per-pixel
 * minimum everywhere.  Columns 0 and W-1 lie outside the Garg crop for W >= 28.
 * The call overwrites every element of depth, whatever it held.  offsets cannot be checked on the host: the kernel clamps
 * every frame's range to [0, total] and takes offsets[b+1] < offsets[b] as an empty frame, so a wrong offset can misassign
 * points but never reads outside points.  Integer atomic minima on the bit patterns in depth itself: no workspace, no
 * allocation, no synchronisation (graph-capturable), and a minimum does not depend on arrival order: two runs are
 * bit-identical.
 * Checked on the host before anything is launched: DVF_ERR_INVALID_ARG for a null pointer (points may be null only when
 * total == 0), points not 16-byte aligned, B, H or W <= 0, total < 0, B * H * W >= 2^31 or a flag bit other than
 * DVF_VD_VELODYNE_DEPTH. */
#define DVF_VD_VELODYNE_DEPTH 1u
int dvf_velodyne_depth(const float *points /* [total][4] */, const int *offsets /* DEVICE, [B+1] */,
                       const double *proj /* DEVICE, [B][3][4] */, float *depth /* [B][H][W] out */, int B, int H, int W, int total,
                       uint32_t flags, void *stream);

/* ---------------------------------------------------------------- odometry evaluation: chained trajectory, KITTI segment errors
 * The device form of odometry_eval.py's se3_cam2world / sequence_errors / overall_error (reference inference.py:63-70,
 * tools/evaluation_tools.py:419-508).  All arithmetic is fp64 and these pointers are DEVICE pointers to DOUBLE data unless
 * stated otherwise.  No allocation, no synchronisation (graph-capturable), no float atomics and a fixed order of every sum:
 * two runs are bit-identical.
 *
 * dvf_pose_chain: rel [N][4][4] fp32 relative poses (the top three rows are read and converted exactly; the fourth is taken
 *   as 0 0 0 1).  offsets is a HOST array of S+1 ints, read and checked at call time and handed to the kernel by value:
 *   sequence s owns rel[offsets[s] .. offsets[s+1]) and writes n_s + 1 camera-to-world poses of 12 doubles (a KITTI pose line)
 *   starting at row offsets[s] + s of world [N+S][3][4]: the identity, then T_k = T_{k-1} * P_k.  An empty sequence writes just
 *   the identity.  The product is an inclusive scan with (R1,t1)*(R2,t2) = (R1 R2, R1 t2 + t1): one 256-thread block per sequence,
 *   every thread multiplies a contiguous chunk, the 256 chunk products are scanned through LDS and a second pass applies the
 *   exclusive prefix.  No re-orthonormalisation (the numpy chain has none); the association differs from the sequential
 *   chain's, an error of about N * 2^-53 relative.
 *   DVF_ERR_INVALID_ARG for a null pointer, S outside 1..32, offsets[0] != 0, a decreasing offset or N = offsets[S] >= 2^24.
 *
 * dvf_odometry_errors: one sequence, dense trajectories gt and res [n][3][4] (frame i = row i of both).  dist = cumulative
 *   path length of gt (ws, n doubles: chunk sums, a block scan and a second pass; within 1e-12 relative of the sequential sum).
 *   For every start frame first = 9, 19, ... < n (nstart of them) and every segment length L = 100, 200 .. 800 m, in that
 *   order, one row of rows [nstart*8][6]: last = the first index after first with dist[last] > dist[first] + L (binary
 *   search), e = inv(d_res) * d_gt with d_x = inv(x[first]) * x[last], and the row is
 *     [first, r_err / L, t_err / L, L, L / (0.1 * (last - first + 1)), 1],   t_err = |e_t|, r_err = acos(clip((tr e_R - 1) / 2));
 *   a pair without such a last gives an all-zero row.  inv is the inverse of the affine [A|t], (A^-1, -A^-1 t) with A^-1 by
 *   cofactors: on an orthonormal A it is the rigid inverse (A^T, -A^T t) up to rounding, and on the chained fp32 outputs of a
 *   network, orthonormal only to ~1e-7, it stays what numpy's general inverse gives.  The angle is the definition's acos form for
 *   the same reason: atan2(|skew part|, trace - 1) equals it only on an exact rotation and differs from it at first order in
 *   e_R's departure from one; near zero the acos form resolves angles down to sqrt(2 eps) ~ 2e-8 rad, far below what a segment
 *   error means.
 *   summary [4] = [sum t_err/L, sum r_err/L, number of valid rows, path length of gt], the rows added in a fixed order;
 *   accumulate != 0 adds the first three to what summary holds (the sums over all sequences of a pass, still one
 *   synchronisation), the fourth is always this sequence's.  n <= 9 has no row: only the summary is written.
 *   DVF_ERR_INVALID_ARG for n < 1, a null pointer (rows may be null when n <= 9) or ws_doubles below the query. */
int dvf_pose_chain(const float *rel /* [N][4][4] */, const int *offsets /* HOST, [S+1] */, int S, double *world /* [N+S][3][4] */,
                   void *stream);
int64_t dvf_odometry_errors_ws_doubles(int n);
int dvf_odometry_errors(const double *gt, const double *res /* [n][3][4] each */, int n, double *rows /* [nstart*8][6] */,
                        double *summary /* [4] */, int accumulate, double *ws, int64_t ws_doubles, void *stream);

/* Alignment of a trajectory to ground truth and the errors of the aligned trajectory: the device form of odometry_eval.py's
 * trajectory_alignment / apply_alignment / trajectory_errors / snippet_errors (reference inference.py:72-88, compute_pose_error,
 * with the scale factor that its line 75 comments out).  Same rules as above; gt and res are dense [n][3][4] trajectories, frame
 * i = row i of both, nothing is re-based.  Sums over the frames are per-block partials (256 frames a block, a fixed LDS tree)
 * in ws, added in block order.  Every entry: DVF_ERR_INVALID_ARG for n < 1 or n >= 2^24, a null pointer, or ws_doubles below the
 * entry's query.
 *
 * dvf_trajectory_align: fits, on the translation columns x_i of res and y_i of gt alone, the transform record
 *   transform [16] = c, R[9] (row-major), t[3], sv[3]   for mode
 *     DVF_ALIGN_NONE        c = 1, R = I, t = 0
 *     DVF_ALIGN_SCALE       c = sum y.x / sum x.x about the origin, uncentred (1 when the denominator is exactly 0), R = I, t = 0
 *     DVF_ALIGN_7DOF        Umeyama: Sigma = 1/n sum (y - my)(x - mx)^T = U D V^T, S = diag(1, 1, sign(det U det V)),
 *                           R = U S V^T, c = tr(D S) / var_x with var_x = 1/n sum |x - mx|^2 (1 when it is exactly 0),
 *                           t = my - c R mx
 *     DVF_ALIGN_6DOF        the same with c = 1
 *     DVF_ALIGN_SCALE_7DOF  c of 7DOF, R = I, t = 0
 *   sv = the singular values of Sigma, descending (zeros for NONE / SCALE): a straight line has sv[1] = sv[2] = 0 and no unique
 *   rotation.  The centred sums are a second pass over the data after the means (a first pass leaves sum x, sum y, sum y.x,
 *   sum x.x), so a common offset of 1e6 m costs nothing.  One thread solves the 3x3 problem by one-sided Jacobi rotations of
 *   Sigma's columns (nothing is squared) and builds R from the two leading singular pairs and their cross products: it is a
 *   proper rotation, orthonormal with determinant +1 to rounding, for every input, rank-deficient ones included (rank 1: an
 *   optimal rotation among the many; Sigma = 0: the identity).  The last three modes need n >= 3; an unknown mode is an error.
 *
 * dvf_trajectory_apply: out_i = [R R_i | c R t_i + t] for every pose of res, one thread per pose; copy != 0 copies res
 *   unchanged and does not read transform (mode NONE).  out may not overlap res.
 *
 * dvf_trajectory_errors: out [4] = [ate, rpe_trans, rpe_rot, n]: ate = sqrt(1/n sum |y_i - x_i|^2); for the n - 1 consecutive
 *   pairs E = inv(inv(gt_i) gt_{i+1}) * (inv(res_i) res_{i+1}), rpe_trans = mean |E_t|, rpe_rot = mean atan2(s, tr E_R - 1) in
 *   radians, s the norm of the three off-diagonal differences of E_R (compute_pose_error's angle, inference.py:82-86: exact down
 *   to zero, where the acos of the trace loses eight digits at 1e-4 rad).  inv is the affine inverse of dvf_odometry_errors.
 *   n = 1: both RPE values are NaN.
 *
 * dvf_snippet_errors: for every start frame i = 0 .. n - length (nrows = n - length + 1 of them, none when n < length) both
 *   length-frame snippets are re-based to their first frame, inv(first) * each, the predicted translations are multiplied by
 *   s = sum g.p / sum p.p over the snippet (1 when the denominator is exactly 0) and rows [nrows][2] gets compute_pose_error's
 *   pair: ate = |all translation differences| / length, re = (sum of the angles of R_g inv(R_p)) / length, the angle as above.
 *   summary [5] = [sum ate, sum ate^2, sum re, nrows, 0], the rows added in a fixed order; accumulate != 0 adds the first four
 *   to what summary holds.  length outside 2..8 is an error; rows may be null when n < length. */
#define DVF_ALIGN_NONE 0
#define DVF_ALIGN_SCALE 1
#define DVF_ALIGN_SCALE_7DOF 2
#define DVF_ALIGN_6DOF 3
#define DVF_ALIGN_7DOF 4
int64_t dvf_trajectory_align_ws_doubles(int n);
int dvf_trajectory_align(const double *gt, const double *res /* [n][3][4] each */, int n, int mode, double *transform /* [16] */,
                         double *ws, int64_t ws_doubles, void *stream);
int dvf_trajectory_apply(const double *res /* [n][3][4] */, const double *transform /* [16] */, int n, int copy,
                         double *out /* [n][3][4] */, void *stream);
int64_t dvf_trajectory_errors_ws_doubles(int n);
int dvf_trajectory_errors(const double *gt, const double *res /* [n][3][4] each */, int n, double *out /* [4] */, double *ws,
                          int64_t ws_doubles, void *stream);
int64_t dvf_snippet_errors_ws_doubles(int n);
int dvf_snippet_errors(const double *gt, const double *res /* [n][3][4] each */, int n, int length, double *rows /* [nrows][2] */,
                       double *summary /* [5] */, int accumulate, double *ws, int64_t ws_doubles, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DVF_HIP_H */
