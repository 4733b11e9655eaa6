/*
 * e2emv.h - C ABI of libe2emv.so: the MI355X (gfx950) implementation of the
 * matcher -> Sinkhorn -> weighted-8-point hot path of barbararoessle/e2e_multi_view_matching.
 *
 * The reference has NO native/FFI seam for this path: the seam is two Python callables,
 *   MultiViewMatcher.forward(data) -> dict      (absent submodule; call sites
 *       helpers.py:246, eval_pairs.py:212, eval_multi_view.py:160)
 *   estimate_relative_pose_w8pt(...) -> (T, info)
 *       (pose_optimization/two_view/estimate_relative_pose.py:84-128)
 * The Python package e2e_multi_view_matching_amd re-creates those callables on top of the
 * entry points below through ctypes (INTEGRATION.md shows the binding).  Every function is
 * extern "C", takes plain pointers and sizes, never throws, and returns 0 or a negative
 * e2emv_status; the message for the last failure of a context is e2emv_last_error().
 *
 * Pointers named d_* are DEVICE pointers (hipMalloc / torch.cuda / e2emv_malloc memory on
 * the context's device).  Everything else is host memory.  `stream` is a hipStream_t passed
 * as void* (NULL = the default stream); all compute calls are asynchronous w.r.t. it.
 * The caller owns every input/output buffer; the library owns only its context (weights,
 * workspace arena grown lazily, never shrunk).  One context per (process, device); calls on
 * one context must be serialised by the caller; different contexts are independent.
 */
#ifndef E2EMV_H
#define E2EMV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the functions declared between this push and its pop are its whole
 * dynamic symbol table (tests/test_host_and_abi.py compares `nm -D` with this header). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define E2EMV_ABI_VERSION 1
#define E2EMV_MAX_TUPLE 8
#define E2EMV_MAX_LAYERS 64
#define E2EMV_MAX_KENC 8

typedef struct e2emv_ctx e2emv_ctx;

typedef enum {
    E2EMV_OK = 0,
    E2EMV_EINVAL = -1, /* bad argument / NULL pointer                                     */
    E2EMV_ENOMEM = -2, /* device or host allocation failed                                */
    E2EMV_EHIP = -3,   /* HIP runtime error (no device, launch failure, ...)              */
    E2EMV_ESHAPE = -4, /* unsupported or inconsistent shape                               */
    E2EMV_ESTATE = -5  /* weights missing / not committed                                 */
} e2emv_status;

/* ---- lifecycle -------------------------------------------------------------------- */
int e2emv_version(void);
/* Fails with E2EMV_EHIP when no gfx950 device is usable: there is NO CPU fallback. */
int e2emv_create(e2emv_ctx** out, int device);
void e2emv_destroy(e2emv_ctx* ctx);
const char* e2emv_last_error(const e2emv_ctx* ctx);

/* ---- memory helpers (so a harness without torch can drive the library) ------------ */
int e2emv_malloc(e2emv_ctx* ctx, void** d_ptr, size_t bytes);
int e2emv_free(e2emv_ctx* ctx, void* d_ptr);
int e2emv_h2d(e2emv_ctx* ctx, void* d_dst, const void* src, size_t bytes, void* stream);
int e2emv_d2h(e2emv_ctx* ctx, void* dst, const void* d_src, size_t bytes, void* stream);
int e2emv_sync(e2emv_ctx* ctx, void* stream);

/* ---- weights ----------------------------------------------------------------------
 * Replaces MultiViewMatcher.load_state_dict (helpers.py:47-52).  Keys are the upstream
 * SuperGlue parameter names the reference's checkpoints use:
 *   kenc.encoder.{0,3,..}.{weight,bias}, kenc.encoder.{1,4,..}.{weight,bias,running_mean,
 *   running_var}, gnn.layers.{i}.attn.proj.{0,1,2}.{weight,bias}, gnn.layers.{i}.attn.merge.*,
 *   gnn.layers.{i}.mlp.{0,3}.*, gnn.layers.{i}.mlp.1.* (BatchNorm), final_proj.*, bin_score,
 *   conf_mlp.{0,3}.*, conf_mlp.1.*   (a leading "module." is stripped).
 * Tensors are host fp32, dense row-major, Conv1d weights [out,in,1] or [out,in].
 * e2emv_commit_weights folds eval-mode BatchNorm into the preceding conv, re-orders the
 * attention channels from upstream's c = dd*H + h to head-major, and uploads.             */
typedef struct {
    int32_t desc_dim;                        /* D, 256                                    */
    int32_t num_heads;                       /* H, 4 (head dim D/H must be 64)            */
    int32_t n_kenc;                          /* hidden keypoint-encoder layers            */
    int32_t kenc[E2EMV_MAX_KENC];            /* [32,64,128,256]                           */
    int32_t n_layers;                        /* L = len(GNN_layers)                       */
    int32_t layer_types[E2EMV_MAX_LAYERS];   /* 0 = 'self', 1 = 'cross'                   */
    int32_t conf_mlp;                        /* 1: conf_mlp.* weights present             */
} e2emv_model_desc;

int e2emv_set_weight(e2emv_ctx* ctx, const char* key, const float* data, const int64_t* shape, int ndim);
int e2emv_commit_weights(e2emv_ctx* ctx, const e2emv_model_desc* model);

/* ---- matcher forward --------------------------------------------------------------
 * Replaces MultiViewMatcher.forward(data) (call sites above).  B tuples of T images with
 * N keypoints each; P = T(T-1)/2 pairs ordered (0,1),(0,2),(1,2),(0,3)... i.e. for j in
 * range(T): for i in range(j) - the order helpers.py:250-251 iterates.                    */
#define E2EMV_FLAG_FULL_OUTPUT 1 /* also produce matches / scores / confidences           */
#define E2EMV_FLAG_MULTI_FRAME 2 /* joint GNN over all T images (cross = all other images) */
#define E2EMV_DESC_F32 0
#define E2EMV_DESC_F16 1

typedef struct {
    int32_t batch;          /* B                                                          */
    int32_t tuple_size;     /* T <= E2EMV_MAX_TUPLE                                       */
    int32_t n_kpts;         /* N (same for every image of the call)                       */
    int32_t sinkhorn_iters; /* 100                                                        */
    float match_threshold;  /* 0.2                                                        */
    int32_t desc_dtype;     /* E2EMV_DESC_F32 | E2EMV_DESC_F16                            */
    int32_t flags;
    float img_w[E2EMV_MAX_TUPLE], img_h[E2EMV_MAX_TUPLE]; /* data['image{m}'].shape[-1/-2] */
    int32_t n_kpts_img[E2EMV_MAX_TUPLE]; /* per-image keypoint count N_m (0 = n_kpts): eval_pairs.py feeds images with
                                            different numbers of SuperPoint keypoints; n_kpts must be the maximum   */
} e2emv_forward_desc;

/* d_kpts[m]   [B,N_m,2] f32 pixel xy      (data['keypoints{m}'])
 * d_kscores[m][B,N_m]   f32               (data['scores{m}'])
 * d_desc[m]   [B,D,N_m] f32|f16, N_m contiguous (data['descriptors{m}'])
 * outputs, one pointer per pair p = (i, j) (any may be NULL = not wanted):
 * d_logZ[p]     [B,N_i+1,N_j+1] f32  result['scores_{i}_{j}']
 * d_matches0[p] [B,N_i] int64    result['matches{i}_{i}_{j}'] (-1 = unmatched; int64 because
 *                                the reference uses it as a fancy index, estimate_relative_pose.py:26-30)
 * d_matches1[p] [B,N_j] int64    result['matches{j}_{i}_{j}']
 * d_mscores0/1[p] [B,N_i]/[B,N_j] f32  matching scores
 * d_conf[p]     [B,N_i] f32      result['conf_scores_{i}_{j}'] (caller views it [B,N_i,1])  */
int e2emv_matcher_forward(e2emv_ctx* ctx, const e2emv_forward_desc* fd,
                          const float* const* d_kpts, const float* const* d_kscores, const void* const* d_desc,
                          float* const* d_logZ, int64_t* const* d_matches0, int64_t* const* d_matches1,
                          float* const* d_mscores0, float* const* d_mscores1, float* const* d_conf,
                          void* stream);

/* ---- Sinkhorn / matching as stand-alone operators ---------------------------------
 * log_optimal_transport(scores, bin_score, iters) of upstream superglue.py (used inside the
 * forward above): d_scores [B,M,N] f32 -> d_logZ [B,M+1,N+1] f32.                         */
int e2emv_sinkhorn(e2emv_ctx* ctx, int B, int M, int N, const float* d_scores, float bin_score, int iters,
                   float* d_logZ, void* stream);
/* mutual arg-max block of SuperGlue.forward on d_logZ [B,M+1,N+1]. */
int e2emv_extract_matches(e2emv_ctx* ctx, int B, int M, int N, const float* d_logZ, float match_threshold,
                          int64_t* d_matches0, int64_t* d_matches1, float* d_mscores0, float* d_mscores1,
                          void* stream);

/* ---- two-view pose ----------------------------------------------------------------
 * get_kpts (estimate_relative_pose.py:16-31): d_kpts1_g[b,n] = d_kpts1[b, matches[b,n]]
 * (index -1 wraps to the last keypoint), d_conf_out = (matches >= 0) * d_conf.             */
int e2emv_gather_matched(e2emv_ctx* ctx, int B, int N0, int N1, const float* d_kpts1, const int64_t* d_matches,
                         const float* d_conf, float* d_kpts1_g, float* d_conf_out, void* stream);

/* estimate_relative_pose_w8pt (estimate_relative_pose.py:84-128).
 * d_kpts0/1 [B,N,2]; d_intr0/1 [B,kdim,kdim] (kdim 3 or 4, or batch-broadcast when
 * intr_batch == 1); d_conf [B,N]; d_T_gt [B,4,4] needed iff choose_closest.
 * Outputs: d_T [B,4,4]; d_kpts0n/d_kpts1n [B,N,2]; d_conf_n [B,N] (normalised weights);
 * d_inliers [B,N] u8 (written iff determine_inliers); d_posdepth [B,N] u8; d_F [B,3,3]
 * (the estimated essential matrix, may be NULL); d_status [B] int32 (bit0: sum(conf)<=1e-6,
 * bit1: non-finite result, bit2: essential matrix of rank < 2 - no usable correspondence; the pose is then finite but
 * arbitrary, like a library SVD's null-space choice in the reference; bit3: see e2emv_w8pt_ragged), may be NULL.  Returns E2EMV_ESHAPE when N < 8 (the Python shim
 * maps that to the reference's (None, None), estimate_relative_pose.py:85-86).             */
int e2emv_w8pt(e2emv_ctx* ctx, int B, int N, const float* d_kpts0, const float* d_kpts1, const float* d_intr0,
               const float* d_intr1, int kdim, int intr_batch, const float* d_conf, int choose_closest,
               const float* d_T_gt, int determine_inliers, float* d_T, float* d_kpts0n, float* d_kpts1n,
               float* d_conf_n, uint8_t* d_inliers, uint8_t* d_posdepth, float* d_F, int32_t* d_status,
               void* stream);

/* e2emv_w8pt on a RAGGED batch: sample b uses its first d_n_per[b] (0 <= n <= N) correspondences; every per-correspondence
 * buffer keeps the row stride N and the rows beyond n read 0 / false in the outputs.  The Hartley statistics of sample b
 * run over its own n rows only (a zero-weight padding row would change them - estimate_relative_pose.py:56-57), which is
 * what lets the pairs of a tuple with different numbers of matches share one launch (bundle_adjust_io.py:98-131).
 * A sample with n < 8 is not solved (the counts may live on the device only, so the caller cannot drop it): d_T = identity,
 * d_F = 0, all its rows read 0 / false, d_status bit3 is set and no other bit. */
int e2emv_w8pt_ragged(e2emv_ctx* ctx, int B, int N, const int32_t* d_n_per, const float* d_kpts0, const float* d_kpts1,
                      const float* d_intr0, const float* d_intr1, int kdim, int intr_batch, const float* d_conf,
                      int choose_closest, const float* d_T_gt, int determine_inliers, float* d_T, float* d_kpts0n,
                      float* d_kpts1n, float* d_conf_n, uint8_t* d_inliers, uint8_t* d_posdepth, float* d_F, int32_t* d_status,
                      void* stream);

/* All T(T-1)/2 pairs of B tuples in ONE solve (the loop of helpers.py:250-258 / bundle_adjust_io.py:62-100 over the pairs
 * of a tuple, batched): pair q enumerates (i, j), i < j, j outer (q = 0: (0,1), 1: (0,2), 2: (1,2), ...).  get_kpts
 * (estimate_relative_pose.py:16-31) of every pair is fused in: d_kpts[t] [B,N,2] and d_intr[t] [intr_batch,kdim,kdim] per
 * image, d_matches[q] [B,N] int64 / d_conf[q] [B,N] per pair (matches of image i in image j, -1 wraps to the last keypoint
 * with weight 0), d_T_gt[q] [B,4,4] per pair when choose_closest.  All images carry the same N (the fixed-shape batches of
 * helpers.py:89-92).  Outputs are pair-major: element (q, b) at index q*B + b of d_T [P*B,4,4], d_kpts0n / d_kpts1n
 * [P*B,N,2], d_conf_n [P*B,N], d_inliers / d_posdepth [P*B,N], d_F [P*B,3,3], d_status [P*B]; semantics per element as
 * e2emv_w8pt.  3 kernel launches + 1 gather instead of 4 per pair.                                                    */
int e2emv_w8pt_tuple(e2emv_ctx* ctx, int B, int T, int N, const float* const* d_kpts, const float* const* d_intr, int kdim,
                     int intr_batch, const int64_t* const* d_matches, const float* const* d_conf, int choose_closest,
                     const float* const* d_T_gt, int determine_inliers, float* d_T, float* d_kpts0n, float* d_kpts1n,
                     float* d_conf_n, uint8_t* d_inliers, uint8_t* d_posdepth, float* d_F, int32_t* d_status, void* stream);

/* d_out[i] = d_mask[i] ? d_x[i] : 0 - the confidence masking between w8pt and the two-view BA
 * (eval_pairs.py:250-251, bundle_adjust_io.py:18-19: confidence[~pos_depth_mask] = 0). */
int e2emv_apply_mask(e2emv_ctx* ctx, int64_t n, const float* d_x, const uint8_t* d_mask, float* d_out, void* stream);

/* normalize (estimate_relative_pose.py:9-14): d_out[b,n] = ((x - cx) / fx, (y - cy) / fy), fp32. */
int e2emv_normalize_kpts(e2emv_ctx* ctx, int B, int N, const float* d_kpts, const float* d_intr, int kdim, int intr_batch,
                         float* d_out, void* stream);

/* T_a_to_b = inv(pose_b) @ pose_a per batch element (helpers.py:219, 254: the relative pose the GT-match builder and
 * the pose losses use), 4x4 row-major, solved in fp64. */
int e2emv_relative_pose(e2emv_ctx* ctx, int B, const float* d_pose_a, const float* d_pose_b, float* d_T_a2b, void* stream);

/* e2emv_pose_errors plus the reference's reductions (compute_pose_error.py:12, 22): d_transl_valid[b] = |t0||t1| > 1e-6,
 * d_means2 (optional) = {mean rotation error over B, mean translation error over the valid entries (NaN if none)}. */
int e2emv_pose_error_means(e2emv_ctx* ctx, int B, const float* d_T, const float* d_T_gt, float* d_rot_err, float* d_transl_err,
                           uint8_t* d_transl_valid, float* d_means2, void* stream);

/* compute_rotation_error / compute_translation_error_as_angle(reduce=False)
 * (compute_pose_error.py:3-22), radians; entries with |t0||t1| <= 1e-6 give 0.             */
int e2emv_pose_errors(e2emv_ctx* ctx, int B, const float* d_T, const float* d_T_gt, float* d_rot_err,
                      float* d_transl_err, void* stream);

/* Two-view Levenberg-Marquardt bundle adjustment: run_bundle_adjust_2_view / BundleAdjustGaussNewton2View.run
 * (estimate_relative_pose.py:138-144, bundle_adjust_gauss_newton_2_view.py:127-201) - the refinement the reference
 * applies to the w8pt pose in its default eval mode.  d_kpts0n/d_kpts1n [B,N,2] intrinsics-normalised keypoints
 * (info["kpts*_norm"]), d_conf [B,N] (entries <= 0 are ignored), d_T_init [B,4,4].  d_T_out [B,4,4] = best pose
 * (copy of d_T_init where d_valid[b] == 0, i.e. fewer than 7 usable matches).                                  */
int e2emv_ba_2view(e2emv_ctx* ctx, int B, int N, const float* d_kpts0n, const float* d_kpts1n, const float* d_conf,
                   const float* d_T_init, int n_iterations, float* d_T_out, uint8_t* d_valid, void* stream);

/* ---- validation targets and loss -----------------------------
 * compute_gt_matches_of_image_pair (helpers.py:121-203): ground-truth matches of a pair from depth maps and the
 * relative pose.  d_kpts0/1 [B,N,2] pixel xy (truncated to integers like the reference), d_K0/1 [B,4,4],
 * d_T0to1 [B,4,4], d_depth0/1 [B,H,W].  Outputs d_indices [B,2,N+1] int64 (slot N = dustbin, -1 = no match) and
 * d_weights [B,2,N+1] f32 - the tensors helpers.py:203 stacks ("gt_indices_i_j", "gt_weights_i_j").            */
int e2emv_gt_matches(e2emv_ctx* ctx, int B, int N, const float* d_kpts0, const float* d_kpts1, const float* d_K0,
                     const float* d_K1, const float* d_T0to1, const float* d_depth0, const float* d_depth1, int H, int W,
                     float max_matched_reproj_err, float min_unmatched_reproj_err, int64_t* d_indices, float* d_weights,
                     void* stream);
/* compute_match_loss (helpers.py:228-241) on d_logZ [B,N+1,N+1] -> d_loss[0] (already divided by B). */
int e2emv_match_loss(e2emv_ctx* ctx, int B, int N, const float* d_logZ, const int64_t* d_indices, const float* d_weights,
                     float* d_loss, void* stream);

/* ---- multi-view pose back-end --------------------------------
 * Global initialisation = the reference's `ba_initializer` executable (bundle_adjustment/ba_init/src/
 * ba_init.cpp:10-90): robust rotation averaging (Chatterjee & Govindu 2013; L1 steps then IRLS) followed by
 * least-unsquared-deviation positions (Ozyesil & Singer 2015).  Two forms of the same solver: the four HOST entry
 * points below (fp64 on one host thread like the reference, <= 64 views, behind the CSV path) and, further down, the
 * DEVICE form for a batch of problems (e2emv_mv_init_batch, e2emv_mv_tuple_init: one wave per problem, <= 8 views).
 * Host form: all pointers are HOST memory, no context needed.  Rotations are COLUMN-major 3x3
 * (the CSV order), world -> camera; pair e = (id0, id1) carries R_021 and the position of camera id1 in the frame of
 * camera id0 (ba_init.cpp:30-50).  View 0 is the gauge.  out_t = -R * position (ba_init.cpp:65).
 * *status: bit 1 = rotation averaging failed, bit 2 = position estimation failed (results then = best so far).      */
int e2emv_mv_init(int n_views, const double* init_R, int n_pairs, const int32_t* pair_ids, const double* pair_R,
                  const double* pair_pos, double* out_R, double* out_t, int32_t* status);
/* The two estimators on their own (angle-axis in/out), as the reference's gtests exercise them
 * (ba_init/test/test_ba_init.cpp:95-268).  rot_aa [n_views,3] is the initial guess on input.                        */
int e2emv_mv_estimate_rotations(int n_views, int n_pairs, const int32_t* pair_ids, const double* pair_rot_aa,
                                double* rot_aa);
int e2emv_mv_estimate_positions(int n_views, int n_pairs, const int32_t* pair_ids, const double* pair_pos,
                                const double* rot_aa, double* out_pos);
/* `ba_init_in.csv` -> `ba_init_out.csv` (ba_initializer.cpp:7-23; wire format ba_init.cpp:13-51, 58-75).           */
int e2emv_mv_init_files(const char* in_csv, const char* out_csv);

/* Weighted reprojection bundle adjustment of <= E2EMV_MAX_TUPLE cameras on the DEVICE = the reference's
 * `bundle_adjuster` executable (problem/include/ba_problem.h:60-151, problem/src/ba_problem.cpp:115-157: Ceres
 * DENSE_SCHUR, squared loss, default options, restated as a Levenberg-Marquardt trust-region loop with an analytic
 * Schur complement; one workgroup runs the whole optimisation).  All pointers are HOST memory (the wire format is
 * CSV / numpy): intr = {fx, fy, cx, cy}; observation o = (cam_idx, pt_idx, obs_xy[2], obs_w[2] = residual weights);
 * cams [n_cams,6] = angle-axis + translation, world -> camera, in/out; pts [n_pts,3] in/out.  The fixed camera is
 * predicted with the IDENTITY pose and its row is returned untouched (ba_problem.cpp:129-137).  summary[4] =
 * {initial cost, final cost, iterations, termination: 0 max-iterations 1 gradient 2 parameter 3 function tolerance,
 * 4 five invalid steps, 5 radius underflow}.  Synchronous.                                                           */
int e2emv_mv_bundle_adjust(e2emv_ctx* ctx, int n_cams, int fixed_cam, int n_pts, int n_obs, const double* intr,
                           const int32_t* cam_idx, const int32_t* pt_idx, const double* obs_xy, const double* obs_w,
                           double* cams, double* pts, int max_iterations, double* summary, void* stream);
/* `ba_in.csv` -> `ba_out.csv` (bundle_adjuster.cpp:7-23; parser ba_problem.cpp:8-88, writer :98-113), 50 iterations. */
/* n_problems such problems solved by ONE kernel launch, one workgroup per problem; e2emv_mv_bundle_adjust is the batch of
 * one, and a problem's result does not depend on its neighbours or its position (bit for bit).  HOST pointers.  Problem k
 * has n_cams[k] cameras (its rows of cams follow those of problem k - 1), fixed camera fixed_cam[k], intrinsics
 * intr[4k..4k+3], the points pt_off[k] .. pt_off[k+1] of pts and the observations obs_off[k] .. obs_off[k+1] of cam_idx /
 * pt_idx / obs_xy / obs_w; cam_idx and pt_idx count from 0 inside their problem.  Offsets start at 0 and do not decrease
 * (E2EMV_ESHAPE); a problem may have no point, and cameras without observations keep their parameters.  summary
 * [n_problems,4] as above (may be NULL).  Synchronous.                                                               */
int e2emv_mv_bundle_adjust_batch(e2emv_ctx* ctx, int n_problems, const int32_t* n_cams, const int32_t* fixed_cam,
                                 const double* intr, const int64_t* pt_off, const int64_t* obs_off, const int32_t* cam_idx,
                                 const int32_t* pt_idx, const double* obs_xy, const double* obs_w, double* cams, double* pts,
                                 int max_iterations, double* summary, void* stream);
/* The reverse pass of e2emv_mv_bundle_adjust_batch (squared loss only).  The inputs of that entry, all HOST; cams and pts are the
 * START values and are read-only.  g_cams [sum C,6] = dLoss/d(cams out), g_pts [sum P,3] = dLoss/d(pts out) (NULL: zeros) ->
 * g_obs_w [sum O,2], g_cams0 [sum C,6], g_pts0 [sum P,3] = dLoss/d(obs_w, cams start, pts start); any output may be NULL.  One
 * workgroup per problem, fp64, one launch: the LM loop is run again from the inputs with a tape behind the solver's workspace (per
 * pass the radius, the solved and the accept flag, per accepted step the iterate before it: max_iterations * (3 + 6 C + 3 P) doubles
 * per problem, sized in size_t - E2EMV_ENOMEM when it cannot be reserved), then the accepted steps are reversed exactly from last to
 * first: the damped system of the step solved by the forward's Schur complement and Cholesky factor with the adjoint as right-hand
 * side, back through the residuals and their analytic Jacobians (second derivatives of the rotation in the branch the forward took).
 * NO GRADIENT is carried by the radius (its rho-dependent update included), the Jacobi scales of the first iterate, the accept /
 * reject comparisons, the termination tests, obs_xy and the intrinsics; a damping that sits on its clamp (1e-6, 1e32) is a
 * constant; an unsolved or rejected step is the identity.  The fixed camera's row and the row of a camera without observations pass
 * through (g_cams0 = g_cams there); a problem that stopped before any accepted step returns g_obs_w = 0, g_cams0 = g_cams, g_pts0
 * = g_pts.  A problem's result does not depend on its neighbours or its position.  Shape errors as in the forward entry.
 * Synchronous.                                                                                                                */
int e2emv_mv_bundle_adjust_batch_backward(e2emv_ctx* ctx, int n_problems, const int32_t* n_cams, const int32_t* fixed_cam,
                                          const double* intr, const int64_t* pt_off, const int64_t* obs_off, const int32_t* cam_idx,
                                          const int32_t* pt_idx, const double* obs_xy, const double* obs_w, const double* cams,
                                          const double* pts, int max_iterations, const double* g_cams, const double* g_pts,
                                          double* g_obs_w, double* g_cams0, double* g_pts0, void* stream);
/* `ba_in.csv` -> `ba_out.csv` (bundle_adjuster.cpp:7-23; parser ba_problem.cpp:8-88, writer :98-113), 50 iterations. */
int e2emv_mv_bundle_adjust_files(e2emv_ctx* ctx, const char* in_csv, const char* out_csv, void* stream);
/* cv2.triangulatePoints as used by write_bundle_adjust_problem (bundle_adjust_io.py:226-227): homogeneous DLT of
 * two views, one thread per point, fp64.  HOST pointers: P0, P1 [3,4] row-major, x0, x1 [n,2], xyz [n,3].           */
int e2emv_mv_triangulate(e2emv_ctx* ctx, int n, const double* P0, const double* P1, const double* x0, const double* x1,
                         double* xyz, void* stream);

/* The multi-view back-end for a whole batch of B tuples of T images without files (the first stage of
 * bundle_adjust_io.py:62-96 for every batch element at once).  Pair q enumerates (i, j), i < j, j outer; problem (b, q) has
 * index b * P + q, P = T (T - 1) / 2.  HOST arrays of P DEVICE pointers: d_kpts0[q] [B,N,2] keypoints of image i,
 * d_kpts1[q] [B,n_kpts1[q],2] keypoints of image j, d_matches[q] [B,N] int64 (NULL: the pair has no matches, count 0),
 * d_conf[q] [B,N,conf_channels].  Keypoint n of image i is kept when 0 <= match < n_kpts1[q] and every confidence channel is
 * > conf_thresh; the kept rows go, IN ASCENDING n, to d_mkpts0 / d_mkpts1 [B*P,N,2] (the keypoint and its match) and d_mconf
 * [B*P,N] (first channel) - the padded layout e2emv_w8pt_ragged reads, rows behind the count 0 - and their number to
 * d_count [B*P].  One launch, no host synchronisation.                                                                  */
int e2emv_mv_collect(e2emv_ctx* ctx, int B, int T, int N, const float* const* d_kpts0, const float* const* d_kpts1,
                     const int32_t* n_kpts1, const int64_t* const* d_matches, const float* const* d_conf, int conf_channels,
                     float conf_thresh, float* d_mkpts0, float* d_mkpts1, float* d_mconf, int32_t* d_count, void* stream);
/* write_bundle_adjust_problem + bundle_adjuster + read_bundle_adjust_result (bundle_adjust_io.py:193-273) for B tuples
 * from the buffers of e2emv_mv_collect, in memory: counts [B*P] HOST copy of d_count; d_intr HOST array of T DEVICE
 * pointers [intr_batch,kdim,kdim] (intr_batch 1 or B, kdim 3 or 4); extr HOST [B,T,4,4] row-major world -> camera start
 * poses.  One launch builds all problems (fp32 (kp - c) / f observations widened to fp64, one DLT point per match, weights
 * = confidence / (0.5 (sum + 1e-3)) with the tuple's sum over its 2 n_pts observations in fp64, index lists in closed
 * form from the counts), one launch solves them (camera 0 fixed, f = 1, c = 0), as e2emv_mv_bundle_adjust_batch would.
 * out_extr HOST [B,T,4,4], summary HOST [B,4] (may be NULL).  Synchronous.                                             */
int e2emv_mv_tuple_ba(e2emv_ctx* ctx, int B, int T, int N, const int32_t* counts, const float* d_mkpts0, const float* d_mkpts1,
                      const float* d_mconf, const float* const* d_intr, int kdim, int intr_batch, const double* extr,
                      int max_iterations, double* out_extr, double* summary, void* stream);
/* The reverse pass of e2emv_mv_tuple_ba (squared loss only): its inputs, and g_out_extr HOST [B,T,4,4] = dLoss/d(out_extr) ->
 * d_gmconf DEVICE [B*P,N] fp32 = dLoss/d(d_mconf), rows behind the count 0.  It goes through the 4x4 <-> angle-axis conversion of the
 * result (the rotation's derivative in the branch its value takes; row 3 of g_out_extr is ignored), the solver backward
 * (e2emv_mv_bundle_adjust_batch_backward's kernel on the problems built on the device), the two observations of a match with their x
 * and y weight, and the weight normalisation conf / (0.5 (2 sum conf + 1e-3)) including the tuple's sum.  CONSTANTS here: the start
 * extrinsics `extr` and the DLT start points made from them - the averaging that produces the start is not differentiable - and the
 * keypoints and intrinsics.  The tape is sized in size_t, E2EMV_ENOMEM when it cannot be reserved.  Errors as e2emv_mv_tuple_ba.
 * Synchronous.                                                                                                                  */
int e2emv_mv_tuple_ba_backward(e2emv_ctx* ctx, int B, int T, int N, const int32_t* counts, const float* d_mkpts0, const float* d_mkpts1,
                               const float* d_mconf, const float* const* d_intr, int kdim, int intr_batch, const double* extr,
                               int max_iterations, const double* g_out_extr, float* d_gmconf, void* stream);
/* The reverse of e2emv_mv_collect for the confidences: d_gmconf DEVICE [B*P,N] = dLoss/d(d_mconf) is scattered to d_gconf, a HOST
 * array of P DEVICE pointers [B,N,conf_channels] (a NULL entry leaves that pair out), with the keep rule and the ascending order of
 * e2emv_mv_collect (same B, T, N, n_kpts1, d_matches, d_conf, conf_channels, conf_thresh): the k-th kept row of a pair block gets slot k
 * in channel 0; rows not kept, the other channels and every row of a pair without matches get 0.  One launch, no host
 * synchronisation.                                                                                                              */
int e2emv_mv_collect_backward(e2emv_ctx* ctx, int B, int T, int N, const int32_t* n_kpts1, const int64_t* const* d_matches,
                              const float* const* d_conf, int conf_channels, float conf_thresh, const float* d_gmconf,
                              float* const* d_gconf, void* stream);
/* The problems e2emv_mv_tuple_ba would solve, copied out instead (HOST, concatenated in the layout
 * e2emv_mv_bundle_adjust_batch takes; tuple b owns n_b = sum of its counts points and 2 n_b observations): cam_idx, pt_idx
 * [2n], obs_xy, obs_w [2n,2], cams [B*T,6], pts [n,3].                                                                  */
int e2emv_mv_tuple_problem(e2emv_ctx* ctx, int B, int T, int N, const int32_t* counts, const float* d_mkpts0,
                           const float* d_mkpts1, const float* d_mconf, const float* const* d_intr, int kdim, int intr_batch,
                           const double* extr, int32_t* cam_idx, int32_t* pt_idx, double* obs_xy, double* obs_w, double* cams,
                           double* pts, void* stream);

/* Track merging (csrc/mvtracks.hip): the pairwise matches of B tuples become tracks, one 3-D point per scene point instead of
 * one per match.  B, T, N, n_kpts1, d_matches, d_conf, conf_channels, conf_thresh as in e2emv_mv_collect.  Node = keypoint n of
 * image t, id t * Nmax + n, Nmax = max(N, n_kpts1[q]) over ALL pairs (the largest keypoint count); edge = every keypoint of the first image of a
 * pair that e2emv_mv_collect keeps, joined to its match; label = the smallest node id of the connected component; track = a
 * component of >= 2 nodes with at most ONE node per image (a component holding two keypoints of one image is a conflict and
 * is dropped).  d_label [B,T,Nmax] int32 DEVICE: the track's label, -1 for a node in no track; d_stats [B,4] int32 DEVICE:
 * {tracks, observations = nodes in tracks, conflict components, edges}.  One workgroup per tuple, labels in LDS; the result
 * does not depend on the batch position or the run.  One launch, no host synchronisation.  LIMIT: T * Nmax <= 16384 nodes
 * (8 images of 2048 keypoints), E2EMV_ESHAPE above it.                                                                   */
int e2emv_mv_tracks(e2emv_ctx* ctx, int B, int T, int N, const int32_t* n_kpts1, const int64_t* const* d_matches,
                    const float* const* d_conf, int conf_channels, float conf_thresh, int32_t* d_label, int32_t* d_stats,
                    void* stream);
/* e2emv_mv_tracks with a repair stage in front of the labelling: instead of losing every component that holds two keypoints
 * of one image, cut its weakest edges.  Edge id e = q * N + n (pair q in e2emv_mv_collect order, row n); every kept edge starts
 * live.  One round: connected components over the live edges; in EVERY conflicting component the live edge with the smallest
 * (confidence of channel 0 compared as floats with <, -0.0 = +0.0; then the smaller edge id) is cut - one per component per
 * round.  The stage ends after `rounds` rounds, or when nothing conflicts; labels, tracks and conflicts are then those of
 * e2emv_mv_tracks over the live edges (a component that still conflicts is dropped, a node without live edge is in no track).
 * d_stats[b] = {tracks, observations, conflict components LEFT, LIVE edges}: cuts = the edge count of rounds 0 minus d_stats[b][3].
 * rounds = 0 gives e2emv_mv_tracks' labels and stats bit for bit.  0 <= rounds <= 64, else E2EMV_EINVAL.  d_label / d_stats go to
 * e2emv_mv_tuple_ba_tracks / e2emv_mv_tuple_problem_tracks unchanged: a node's confidence there stays the mean over the KEPT
 * edges between it and the other members of its track, so a cut edge whose ends land in one valid track still counts.  One
 * workgroup per tuple, labels, arg-min keys and the dead-edge bitmap in LDS; no floating-point atomics, the result does not depend
 * on the batch position or the run.  One launch, no host synchronisation.  Same LIMIT of 16384 nodes, E2EMV_ESHAPE above it. */
int e2emv_mv_tracks_repair(e2emv_ctx* ctx, int B, int T, int N, const int32_t* n_kpts1, const int64_t* const* d_matches,
                           const float* const* d_conf, int conf_channels, float conf_thresh, int rounds, int32_t* d_label,
                           int32_t* d_stats, void* stream);
/* The counterpart of e2emv_mv_tuple_ba on the tracks: d_label [B,T,Nmax] DEVICE and stats [B,4] HOST copy of d_stats from
 * e2emv_mv_tracks on the same matches / confidences / threshold; d_kpts HOST array of T DEVICE pointers [B,n_kpts[t],2]
 * (the per-image keypoints), n_kpts HOST [T] (<= Nmax; the first image of a pair with matches has >= N); intrinsics and extr
 * as in e2emv_mv_tuple_ba.  One launch builds every tuple's problem: points = tracks in ascending label, the observations
 * of a point in ascending image, concatenated in point order, index lists as e2emv_mv_bundle_adjust_batch builds them;
 * observation = fp32 (kp - c) / f widened to fp64; weight = c / (0.5 (sum + 1e-3)), c the fp64 mean of the node's kept
 * edges' confidences (channel 0, other image ascending), sum over the tuple's observations in a fixed order; start point =
 * homogeneous DLT over the track's k views (for k = 2 the routine of e2emv_mv_triangulate).  One launch solves them (camera
 * 0 fixed, f = 1, c = 0).  A tuple without tracks returns its start.  out_extr HOST [B,T,4,4], summary HOST [B,4] (may
 * be NULL).  Synchronous.                                                                                               */
int e2emv_mv_tuple_ba_tracks(e2emv_ctx* ctx, int B, int T, int N, int Nmax, const int32_t* d_label, const int32_t* stats,
                             const float* const* d_kpts, const int32_t* n_kpts, const int64_t* const* d_matches,
                             const float* const* d_conf, int conf_channels, float conf_thresh, const float* const* d_intr,
                             int kdim, int intr_batch, const double* extr, int max_iterations, double* out_extr,
                             double* summary, void* stream);
/* The problems e2emv_mv_tuple_ba_tracks would solve, copied out instead (HOST, concatenated in the layout
 * e2emv_mv_bundle_adjust_batch takes; tuple b owns stats[b][0] points and stats[b][1] observations): cam_idx, pt_idx [O],
 * obs_xy, obs_w [O,2], cams [B*T,6], pts [P,3].                                                                         */
int e2emv_mv_tuple_problem_tracks(e2emv_ctx* ctx, int B, int T, int N, int Nmax, const int32_t* d_label, const int32_t* stats,
                                  const float* const* d_kpts, const int32_t* n_kpts, const int64_t* const* d_matches,
                                  const float* const* d_conf, int conf_channels, float conf_thresh, const float* const* d_intr,
                                  int kdim, int intr_batch, const double* extr, int32_t* cam_idx, int32_t* pt_idx,
                                  double* obs_xy, double* obs_w, double* cams, double* pts, void* stream);
/* The reverse pass of e2emv_mv_tuple_ba_tracks (squared loss only): its inputs - the SAME d_label and stats the forward ran with - and
 * g_out_extr HOST [B,T,4,4] = dLoss/d(out_extr) -> d_gconf, a HOST array of P DEVICE pointers [B,N,conf_channels] fp32 = dLoss/d(d_conf)
 * (a NULL entry leaves that pair out; every element of the others is written, the caller need not clear them).  It goes through the
 * 4x4 <-> angle-axis conversion and the solver backward as e2emv_mv_tuple_ba_backward does, then through the track weights: with c_o the
 * mean of the e_o kept edges between observation o's node and the other members of its track, H = 0.5 (sum c_o + 1e-3), w_o = c_o / H,
 * G_o the sum of the two dLoss/dw of o and D = sum G_o w_o:  cbar_o = (G_o - D / 2) / H,  and an edge whose two nodes carry the same
 * label >= 0 gets cbar / e of its one node + cbar / e of the other in channel 0 - a cut edge inside its final track included.  Exactly 0:
 * rows the keep rule drops, edges of unlabelled nodes (dropped conflicts), edges between two tracks, the other channels, every row of a
 * tuple without tracks.  FROZEN: labels, keep rule, cuts, and what the solver backward freezes.  CONSTANTS: extr, the DLT start points,
 * keypoints and intrinsics.  One workgroup per tuple, fp64, no atomics: the same words alone, at any batch position and run to run.
 * Errors as e2emv_mv_tuple_ba_tracks; E2EMV_EINVAL for a NULL g_out_extr / d_gconf; the tape is sized in size_t, E2EMV_ENOMEM when it
 * cannot be reserved.  Synchronous.                                                                                            */
int e2emv_mv_tuple_ba_tracks_backward(e2emv_ctx* ctx, int B, int T, int N, int Nmax, const int32_t* d_label, const int32_t* stats,
                                      const float* const* d_kpts, const int32_t* n_kpts, const int64_t* const* d_matches,
                                      const float* const* d_conf, int conf_channels, float conf_thresh, const float* const* d_intr,
                                      int kdim, int intr_batch, const double* extr, int max_iterations, const double* g_out_extr,
                                      float* const* d_gconf, void* stream);

/* Robust loss in the multi-view bundle adjustment: a ceres::LossFunction where the reference passes NULL
 * (ba_problem.cpp:135,144).  One residual block = one observation; s = rx^2 + ry^2 of the WEIGHTED residual; the cost is
 * 1/2 sum rho(s) (also summary[0] and [1]); the linearisation is Ceres' corrector with rho'' <= 0: residual and both Jacobian
 * blocks of the observation times sqrt(rho'(s)); the trust-region loop, its tolerances and termination codes are unchanged.
 *   E2EMV_LOSS_HUBER  a: rho = s, rho' = 1 for s <= a^2, else rho = 2 a sqrt(s) - a^2, rho' = a / sqrt(s)
 *   E2EMV_LOSS_CAUCHY a: rho = a^2 log1p(s / a^2), rho' = 1 / (1 + s / a^2)
 * E2EMV_EINVAL for another code, or with a loss for a scale that is not finite and > 0.  E2EMV_LOSS_NONE ignores the scale
 * and is the entry point without the suffix, launch for launch and bit for bit.                                          */
#define E2EMV_LOSS_NONE 0
#define E2EMV_LOSS_HUBER 1
#define E2EMV_LOSS_CAUCHY 2
/* e2emv_mv_bundle_adjust_batch with a loss; loss_scale = a in the units of the weighted residual, as in Ceres.          */
int e2emv_mv_bundle_adjust_batch_loss(e2emv_ctx* ctx, int n_problems, const int32_t* n_cams, const int32_t* fixed_cam,
                                      const double* intr, const int64_t* pt_off, const int64_t* obs_off, const int32_t* cam_idx,
                                      const int32_t* pt_idx, const double* obs_xy, const double* obs_w, double* cams, double* pts,
                                      int max_iterations, double* summary, int loss, double loss_scale, void* stream);
/* e2emv_mv_tuple_ba / e2emv_mv_tuple_ba_tracks with a loss.  Their weights are confidence / half_total with a per-tuple
 * half_total (0.5 (2 sum + 1e-3) over the matches, 0.5 (sum + 1e-3) over the track observations), so loss_scale is RELATIVE:
 * tuple b runs with a_b = loss_scale / half_total_b - one fp64 division on the device by the denominator of its weights -
 * and the loss acts on confidence x residual in normalised image coordinates: loss_scale = "pixels / focal length at
 * confidence 1" whatever the tuple's size.  loss_a_out HOST [B] (may be NULL): the a_b used (0 without a loss).              */
int e2emv_mv_tuple_ba_loss(e2emv_ctx* ctx, int B, int T, int N, const int32_t* counts, const float* d_mkpts0, const float* d_mkpts1,
                           const float* d_mconf, const float* const* d_intr, int kdim, int intr_batch, const double* extr,
                           int max_iterations, double* out_extr, double* summary, int loss, double loss_scale, double* loss_a_out,
                           void* stream);
int e2emv_mv_tuple_ba_tracks_loss(e2emv_ctx* ctx, int B, int T, int N, int Nmax, const int32_t* d_label, const int32_t* stats,
                                  const float* const* d_kpts, const int32_t* n_kpts, const int64_t* const* d_matches,
                                  const float* const* d_conf, int conf_channels, float conf_thresh, const float* const* d_intr,
                                  int kdim, int intr_batch, const double* extr, int max_iterations, double* out_extr,
                                  double* summary, int loss, double loss_scale, double* loss_a_out, void* stream);
/* e2emv_ba_2view with a loss: the two-view stage robust in the same way.  A residual block is one observation, so a match has
 * two: s0 = |r0|^2 in image 0 and s1 = |r1|^2 in image 1, on the weighted residuals (weight = conf / cden_b, cden_b = 0.5
 * max(2 sum conf, 1e-6) over the pair's positive confidences).  The cost that the LM loop compares - improvement, best pose,
 * lambda - is sum rho(s0) + sum rho(s1); the corrector scales r0 and its point block by sqrt(rho'(s0)), r1 and its point and
 * camera blocks by sqrt(rho'(s1)); the loop itself (update always applied, n_iterations + 1 evaluations, a singular system
 * skips the update) is unchanged.  loss_scale is RELATIVE as above: pair b runs with a_b = loss_scale / cden_b, one fp64
 * division on the device.  d_summary DEVICE [B][4] (may be NULL): cost at the start, best cost, number of evaluations that
 * improved, a_b used (0 without a loss); all zero for a pair with d_valid[b] == 0.  E2EMV_LOSS_NONE with d_summary == NULL is
 * e2emv_ba_2view, launch for launch and bit for bit; shape errors as there.                                                 */
int e2emv_ba_2view_loss(e2emv_ctx* ctx, int B, int N, const float* d_kpts0n, const float* d_kpts1n, const float* d_conf,
                        const float* d_T_init, int n_iterations, float* d_T_out, uint8_t* d_valid, int loss, double loss_scale,
                        double* d_summary, void* stream);
/* The reverse pass of e2emv_ba_2view (squared loss only): d_gT [B,4,4] = dLoss/d(d_T_out) -> d_gconf [B,N] = dLoss/d(d_conf) and
 * d_gTinit [B,4,4] = dLoss/d(d_T_init); either output may be NULL.  One workgroup per pair, fp64: the LM loop is run again from the
 * inputs with a tape in the workspace (the points and the step of every evaluation; (n_iterations + 1) * N * 3 doubles per pair, sized
 * in size_t - E2EMV_ENOMEM when it cannot be reserved), then the steps k* - 1 .. 0 are reversed exactly, k* = the evaluation whose
 * pose became d_T_out: the damped Schur system of the step solved with the adjoint as right-hand side, back through the residuals
 * and Jacobians, the exponential with its |w|^2 >= 1e-4 clamp, the DLT triangulation of the start points and the normalisation of
 * the weights.  lambda, the accept / reject comparisons and k* depend on comparisons only and carry no gradient; a skipped
 * (singular) step is the identity.  Rows with d_conf <= 0 get 0; keypoints carry no gradient; row 3 of d_gTinit is 0 (the forward
 * reads rows 0-2 of d_T_init only).  A pair with d_valid[b] == 0, n_iterations == 0 or no improving evaluation (k* = 0) returned
 * d_T_init: d_gconf = 0, d_gTinit = rows 0-2 of d_gT.  Shape errors as in e2emv_ba_2view.                                   */
int e2emv_ba_2view_backward(e2emv_ctx* ctx, int B, int N, const float* d_kpts0n, const float* d_kpts1n, const float* d_conf,
                            const float* d_T_init, int n_iterations, const float* d_gT, float* d_gconf, float* d_gTinit,
                            void* stream);
/* The reverse pass of e2emv_ba_2view_loss: e2emv_ba_2view_backward for a loop that ran with a robust loss.  loss and loss_scale are
 * those of the forward call (checked the same way, same errors); the loop is replayed with them, so the accept / reject / skip
 * decisions and k* are the forward's.  The step that is reversed solves the CORRECTED system, and the adjoint goes on through
 * the corrector - sqrt(rho'(s)) of each observation block depends on the block's residual and on the pair's scale - and through
 * the scale itself: a_b = loss_scale / cden_b moves with the confidences, and every row with d_conf > 0 receives that term
 * (nothing where cden_b is the 1e-6 clamp).  rho, the costs that are compared, carries no gradient; Huber's kink s = a^2 takes the
 * quadratic branch.  Same workspace, outputs (either may be NULL), shape, NULL and tape-overflow rules as e2emv_ba_2view_backward;
 * E2EMV_LOSS_NONE is e2emv_ba_2view_backward, launch for launch and bit for bit.                                               */
int e2emv_ba_2view_loss_backward(e2emv_ctx* ctx, int B, int N, const float* d_kpts0n, const float* d_kpts1n, const float* d_conf,
                                 const float* d_T_init, int n_iterations, int loss, double loss_scale, const float* d_gT,
                                 float* d_gconf, float* d_gTinit, void* stream);

/* The global initialisation on the DEVICE (csrc/mvinit_device.hip): the solver of e2emv_mv_init with the same options,
 * fp64, one wave per problem, the problem and its working set in LDS; a problem's result depends on neither its
 * neighbours nor its position in the batch (bit for bit), and agrees with the host form to rounding (summation orders
 * differ).  n_problems problems in the array form of e2emv_mv_init, HOST pointers, concatenated, one launch, synchronous:
 * problem k has n_views[k] views (1..E2EMV_MAX_TUPLE; its rows of init_R / out_R [.,9] column-major and out_t [.,3]
 * follow those of problem k - 1) and the pairs pair_off[k] .. pair_off[k+1] (at most 28, each unordered pair of views at
 * most once) of pair_ids [.,2] / pair_R [.,9] / pair_pos [.,3]; ids count from 0 inside their problem.  status
 * [n_problems] as *status of e2emv_mv_init (may be NULL).  A problem without pairs returns its initial rotations and zero
 * translations.  E2EMV_EINVAL: n_views outside 1..8, an id outside its problem or i == j, a repeated pair, a NULL array,
 * offsets that decrease or do not start at 0.                                                                          */
int e2emv_mv_init_batch(e2emv_ctx* ctx, int n_problems, const int32_t* n_views, const double* init_R, const int64_t* pair_off,
                        const int32_t* pair_ids, const double* pair_R, const double* pair_pos, double* out_R, double* out_t,
                        int32_t* status, void* stream);
/* The whole initialisation stage of the batched path for B tuples of T images (2..E2EMV_MAX_TUPLE) on DEVICE buffers,
 * one launch, no host synchronisation: d_rel_T [B*P,16] fp32 row-major 4x4 relative poses (the output of the w8pt +
 * two-view-BA stage), d_n_inliers, d_count [B*P] int32, pair order as in e2emv_mv_collect.  Per tuple: pairs with count >=
 * min_matches are edges weighted by their count; camera-to-world poses are chained from image 0 along the maximum spanning
 * tree (Kruskal in descending weight; EQUAL weights in ascending row-major (i, j) - this library's rule, other spanning
 * tree codes order ties differently) with pose_j = pose_i inv(T_ij), pose_i = pose_j T_ij, every inverse a real fp64
 * matrix inverse (the fp32 rotation blocks are orthonormal to 1e-7 only); the initial rotations are those of the inverted
 * chained poses, the identity for images not reached from image 0; the pairs with n_inliers >= min_inliers or on the tree
 * enter the solver with R_ij and the position -R_ij^T t_ij.  d_extr [B,T,16] fp64 row-major world -> camera, camera 0 the
 * gauge; d_status [B] int32 as *status of e2emv_mv_init.                                                                */
int e2emv_mv_tuple_init(e2emv_ctx* ctx, int B, int T, const float* d_rel_T, const int32_t* d_n_inliers, const int32_t* d_count,
                        int min_matches, int min_inliers, double* d_extr, int32_t* d_status, void* stream);

/* ---- RANSAC essential matrix (SuperGlue's estimate_pose: OpenCV findEssentialMat(RANSAC) + recoverPose) ------------
 * A ragged batch of P problems in one call, no host synchronisation inside: problem p uses its first d_n_per[p]
 * (0 <= n <= Mmax <= 4096) rows of d_kpts0n / d_kpts1n [P,Mmax,2] fp64, keypoints already NORMALISED by their
 * intrinsics, and the normalised threshold d_thresh[p] (fp64).  RANSAC with the 5-point solver: up to max_iters
 * iterations (upstream: 1000), confidence conf; a match is an inlier of E iff its squared Sampson distance is
 * <= thresh^2; a model replaces the best only with strictly more inliers than max(best, 4), and every new best lowers the
 * iteration count to RANSACUpdateNumIters(conf, outlier share, 5, count).  n == 5: no sampling, every solution of the
 * minimal problem is a candidate and the mask is all ones.  Then recoverPose (distance threshold 1e9) of each candidate,
 * restricted to the mask; the candidate with the most points in front of both cameras is kept, only if that count > 0.
 * Sample stream: iteration i draws d = 0, 1, 2, ... -> index floor(h * n / 2^32),
 *   h = mix(mix(mix(seed ^ 0x9E3779B9) ^ i) ^ d),  mix(x): x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16
 * (uint32 arithmetic), an index equal to an earlier pick of the iteration is drawn again; 64 draws without 5 distinct
 * picks leave the iteration without a model.  The batch position is not an input: a problem's result does not depend on
 * the other problems.
 * Outputs per problem: d_E, d_R [P,3,3], d_t [P,3] fp64 (zeros unless status 0); d_inliers [P,Mmax] u8 the RANSAC inlier
 * mask (padding rows 0); d_n_inliers its count; d_n_cheiral recoverPose's count of the kept candidate; d_iters the
 * RANSAC iterations run (1 for n == 5); d_status 0 ok, 1 fewer than 5 matches, 2 RANSAC found no model, 3 no candidate
 * with a point in front of both cameras, 4 n outside [0, Mmax]. */
int e2emv_essential_ransac(e2emv_ctx* ctx, int P, int Mmax, const int32_t* d_n_per, const double* d_kpts0n, const double* d_kpts1n,
                           const double* d_thresh, double conf, int max_iters, uint32_t seed, double* d_E, double* d_R, double* d_t,
                           uint8_t* d_inliers, int32_t* d_n_inliers, int32_t* d_n_cheiral, int32_t* d_iters, int32_t* d_status,
                           void* stream);
/* The RANSAC relative-pose methods on the batched multi-view path (csrc/mvransac.hip): the device glue between
 * e2emv_mv_collect, e2emv_essential_ransac, e2emv_ba_2view and e2emv_mv_tuple_init / e2emv_mv_tuple_ba.  B tuples of T
 * images (2..E2EMV_MAX_TUPLE), problem (b, q) at index b * P + q as in e2emv_mv_collect; DEVICE buffers except d_intr, the
 * HOST array of T DEVICE pointers [intr_batch,kdim,kdim] of e2emv_mv_tuple_ba; one launch each, one workgroup per problem,
 * no host synchronisation.  N > 4096 (the RANSAC's limit): E2EMV_ESHAPE.
 * prepare = ransac.normalize_keypoints + the threshold of estimate_poses_ransac, to the bit: the first d_count[p] rows of
 * d_mkpts0 / d_mkpts1 [B*P,N,2] fp32 pixels -> d_kpts0n / d_kpts1n [B*P,N,2] fp64, (x - K[.,2]) / K[.,.] with keypoint
 * and intrinsic widened to fp64 first (image i of the pair for kpts0, image j for kpts1; rows behind the count 0), and
 * d_thresh [B*P] fp64 = thresh / ((((K_i[0,0] + K_j[1,1]) + K_i[0,0]) + K_j[1,1]) / 4) (upstream's mean, thresh in
 * pixels, upstream: 1.0): what e2emv_essential_ransac reads.                                                            */
int e2emv_mv_ransac_prepare(e2emv_ctx* ctx, int B, int T, int N, const float* d_mkpts0, const float* d_mkpts1,
                            const int32_t* d_count, const float* const* d_intr, int kdim, int intr_batch, double thresh,
                            double* d_kpts0n, double* d_kpts1n, double* d_thresh, void* stream);
/* filter = what initialize_bundle_adjust does with a RANSAC result (bundle_adjust_io.py:104-133): the collected buffers, the
 * outputs of prepare and d_inliers [B*P,N] / d_n_inliers / d_R / d_t / d_status of e2emv_essential_ransac (Mmax = N) ->
 * (a) d_fkpts0 / d_fkpts1 [B*P,N,2], d_fconf [B*P,N] fp32: the rows of a solved problem (status 0) reduced to its inliers IN
 *     THEIR ORDER; a problem that was not solved keeps all its rows (the reference filters only on success and hands every
 *     match of the tuple to the bundle adjustment);
 * (b) d_fkpts0n / d_fkpts1n / d_fconfn, all three or all NULL: the same rows of the NORMALISED keypoints as fp32 (the fp64
 *     value rounded once) and their confidences, 0 for a problem that was not solved - the input of e2emv_ba_2view, which
 *     leaves such a problem at its start;
 * (c) d_T0 [B*P,4,4] fp32 row-major: R | t rounded from fp64, bottom row 0 0 0 1; the identity unless solved;
 * (d) d_ba_count [B*P]: rows in use of (a) = d_n_inliers if solved, else d_count;
 * (e) d_graph_w [B*P]: match-graph weight = d_n_inliers if solved, else 0 (no edge).
 * Rows behind d_ba_count are 0 in (a) and (b).  The outputs must not alias the inputs.                                  */
int e2emv_mv_ransac_filter(e2emv_ctx* ctx, int B, int T, int N, const float* d_mkpts0, const float* d_mkpts1,
                           const float* d_mconf, const int32_t* d_count, const double* d_kpts0n, const double* d_kpts1n,
                           const uint8_t* d_inliers, const int32_t* d_n_inliers, const double* d_R, const double* d_t,
                           const int32_t* d_status, float* d_fkpts0, float* d_fkpts1, float* d_fconf, float* d_fkpts0n,
                           float* d_fkpts1n, float* d_fconfn, float* d_T0, int32_t* d_ba_count, int32_t* d_graph_w,
                           void* stream);
/* The 5-point minimal solver alone: n problems of 5 normalised correspondences d_x0, d_x1 [n,5,2] fp64 -> every real
 * essential matrix, d_E [n,10,3,3] (unit Frobenius norm, rows beyond d_nsol[i] zero), d_nsol [n] int32 (0..10). */
int e2emv_essential_5pt(e2emv_ctx* ctx, int n, const double* d_x0, const double* d_x1, double* d_E, int32_t* d_nsol, void* stream);

/* ---- SuperPoint front-end --------------------------------------
 * Replaces models.models.superpoint.SuperPoint (absent submodule; call sites helpers.py:73-96, configs train.py:335-341,
 * eval_pairs.py:197-202, eval_multi_view.py:135-140) = upstream magicleap SuperPoint.  Weights go in through
 * e2emv_set_weight with the upstream parameter names prefixed by "superpoint." (superpoint.conv1a.weight [64,1,3,3] ...
 * superpoint.convDb.bias [256]; layers conv1a conv1b conv2a conv2b conv3a conv3b conv4a conv4b convPa convPb convDa
 * convDb), then e2emv_superpoint_commit repacks them for NHWC implicit-GEMM convolutions.                          */
typedef struct {
    int32_t batch;             /* images in this call (a merged tuple batch, helpers.py:73-81)                      */
    int32_t height, width;     /* multiples of 8 (the storage grid; see valid_height / valid_width)                   */
    int32_t nms_radius;        /* config "nms_radius"                                                                 */
    int32_t max_keypoints;     /* K: capacity of the outputs, 1..4096 (config "max_keypoints"; -1 is mapped by the
                                  Python layer to the capacity)                                                       */
    int32_t remove_borders;    /* config "remove_borders"                                                             */
    int32_t fill_random;       /* fork option "fill_with_random_keypoints": pad to K with pseudo-random pixels        */
    float keypoint_threshold;  /* config "keypoint_threshold"                                                         */
    uint32_t seed;             /* for fill_random                                                                     */
    int32_t valid_height, valid_width; /* 0 = height / width.  Otherwise the size of the images themselves, stored zero-padded
                                  on the (height, width) grid with height - valid_height < 8 (same for the width): the
                                  convolutions see the whole image and every max-pool floors, like upstream            */
} e2emv_superpoint_desc;
int e2emv_superpoint_commit(e2emv_ctx* ctx);
/* d_images [B,H,W] fp32 grey in [0,1].  Outputs: d_kpts [B,K,2] pixel (x, y), d_scores [B,K], d_desc [B,256,K]
 * (descriptor-major, what the matcher's descriptors{m} input wants), d_count [B] valid entries per image (the rest is
 * zero).  Order: row-major when an image has <= K candidates, else score-descending (ties: lower pixel index).
 * d_score_map (optional) [B,H8,W8] (H8 = valid height rounded down to a multiple of 8) receives the NMS-ed score map.                                                        */
int e2emv_superpoint_forward(e2emv_ctx* ctx, const e2emv_superpoint_desc* desc, const float* d_images, float* d_kpts,
                             float* d_scores, float* d_desc, int32_t* d_count, float* d_score_map, void* stream);

/* ---- building blocks exported for per-kernel parity tests and micro-benchmarks ----- */
/* C[z][m][n] = act(sum_k A[z][m][k] W[z][n][k] * scale + bias[n]) (+ R[z][m][n]); all f32;
 * A may be split in two K-segments (A: k < K1, A2: K1 <= k < K).  flags: bit0 relu.        */
int e2emv_gemm_nt(e2emv_ctx* ctx, int batch, int M, int Nout, int K, int K1, const float* d_A, int64_t lda,
                  int64_t strideA, const float* d_A2, int64_t lda2, int64_t strideA2, const float* d_W,
                  int64_t ldw, int64_t strideW, const float* d_bias, const float* d_R, int64_t ldr,
                  int64_t strideR, float* d_C, int64_t ldc, int64_t strideC, float scale, int flags,
                  void* stream);
/* Multi-head attention over head-major channels: d_qkv [n_img, n_rows, 3*D] (q|k|v), image
 * g = b*T + t attends to itself (cross == 0) or to every other image of its tuple;
 * n_valid keys/queries per image; output d_out [n_img, n_rows, D].                         */
int e2emv_attention(e2emv_ctx* ctx, int B, int T, int n_rows, int n_valid, int D, int H, const float* d_qkv,
                    int cross, float* d_out, void* stream);
/* The same with a keypoint count per image of a tuple, as the matcher forward runs the kernel on images whose counts differ:
 * n_valid_per_image = HOST array of T ints (1 .. n_rows each; E2EMV_ESHAPE otherwise, E2EMV_EINVAL for NULL or
 * T > E2EMV_MAX_TUPLE, nothing launched); image g = b*T + t has n_valid_per_image[t] queries and, as a source, that many
 * keys.  Output rows at and beyond an image's count are written as zeros or not written. */
int e2emv_attention_v(e2emv_ctx* ctx, int B, int T, int n_rows, const int* n_valid_per_image, int D, int H,
                      const float* d_qkv, int cross, float* d_out, void* stream);

/* Three stages of the training path (e2emv_matcher_forward_train / e2emv_matcher_backward, below) alone, each through the
 * host function the product calls.  All fp32 device buffers.  None needs e2emv_train_commit; scratch is the context's
 * workspace; a tape held by the context is left as it is.  Arguments the product cannot produce are E2EMV_ESHAPE /
 * E2EMV_EINVAL before any launch.
 *
 * Backward of a dense layer y = x W^T + b over `rows` rows: d_dY [rows][ldy] (n_out columns used), d_X [rows][ldx] (n_in
 * used), d_W [n_out][ldw].  d_dW [n_out][ldw] += dY^T X and d_db [n_out] += column sums of dY (the caller zeroes both, as the
 * backward zeroes its gradient arena); d_dX (optional) [rows][ldx] = dY W, added to when accumulate != 0. */
int e2emv_train_linear_backward(e2emv_ctx* ctx, int64_t rows, int n_out, int n_in, const float* d_dY, int64_t ldy,
                                const float* d_X, int64_t ldx, const float* d_W, int64_t ldw, float* d_dW, float* d_db,
                                float* d_dX, int accumulate, void* stream);
/* The unrolled log-domain Sinkhorn with its tape, B problems of N x N scores d_S [B][N][ldS] (N 1..2048, ldS >= N), dustbin
 * score alpha: d_logZ [B][N+1][N+1]; d_uv (optional) [B][iters+1][2][N+1] = u_t, v_t of every iteration (t = 0: zeros).
 * With d_G = dLoss / dlogZ [B][N+1][N+1] also the reverse sweep: d_dC [B][N+1][N+1] = dLoss / d couplings (its dustbin row
 * and column included) and d_dalpha [1] = their sum over all problems.  col_width: columns per workgroup of the two column
 * kernels, 32 or 64; 0 = the product's rule (64 once B * ceil((N+1)/64) workgroups fill the chip). */
int e2emv_train_sinkhorn(e2emv_ctx* ctx, int B, int N, const float* d_S, int64_t ldS, float alpha, int iters, int col_width,
                         const float* d_G, float* d_logZ, float* d_uv, float* d_dC, float* d_dalpha, void* stream);
/* Backward of e2emv_attention (head dim 64: D = 64 H): d_qkv [B*T][n_rows][3D] and d_datt = dLoss / d out [B*T][n_rows][D]
 * with n_rows = N rounded up to a multiple of 128, N (1..2048) valid rows per image, T in 2..E2EMV_MAX_TUPLE ->
 * d_dqkv [B*T][n_rows][3D]; rows N..n_rows of an image are not read and come back as zeros. */
int e2emv_train_attention_backward(e2emv_ctx* ctx, int B, int T, int N, int D, int H, int cross, const float* d_qkv,
                                   const float* d_datt, float* d_dqkv, void* stream);

/* The SuperPoint detector tail alone, on a score map the caller supplies: simple_nms -> threshold -> border removal -> top-k,
 * and (if d_dense is given) the descriptor sampling - the kernels, launch geometry and order e2emv_superpoint_forward runs
 * behind its detector and descriptor heads.  desc as for forward (height, width = size of the score map: multiples of 8, at
 * least 16; valid_height / valid_width 0 or equal to them; max_keypoints 1..4096; nms_radius 0..16); needs no committed
 * weights.  Outputs as for forward: entries beyond d_count[b] are zero.                                               */
int e2emv_superpoint_detect(e2emv_ctx* ctx, const e2emv_superpoint_desc* desc,
                            const float* d_score,  /* [B,H,W] fp32: the map simple_nms receives                        */
                            const float* d_dense,  /* optional [B,H/8,W/8,256] NHWC: the UNnormalised descriptor-head output */
                            float* d_kpts, float* d_scores, int32_t* d_count,
                            float* d_desc,         /* [B,256,K]; required if and only if d_dense is given               */
                            float* d_nms_map,      /* optional [B,H,W]: the NMS-ed map                                  */
                            void* stream);
/* The head of e2emv_superpoint_forward alone, image -> score map + dense descriptors: everything in front of the detector tail
 * and the descriptor sampling, by the same host function (one list of launches).  desc as for forward; its detector fields
 * (nms_radius, max_keypoints, remove_borders, fill_random, keypoint_threshold, seed) are ignored.  Needs committed weights.
 * d_taps: optional HOST array of 12 DEVICE pointers (NULL entries are skipped); tap l receives the output of layer l (conv1a ..
 * convDb in the order of e2emv_superpoint_commit) exactly as the next stage reads it - after the fused 2x2 max-pool, after the
 * masking to the valid size and, for layer 5, after the crop to the cell grid - by a device-to-device copy on the stream.  With
 * (Hp, Wp) = (height, width) and (Hc, Wc) = (valid height / 8, valid width / 8) floored, all NHWC fp32:
 * 0 [B,Hp,Wp,64]; 1, 2 [B,Hp/2,Wp/2,64]; 3 [B,Hp/4,Wp/4,64]; 4 [B,Hp/4,Wp/4,128]; 5, 6, 7 [B,Hc,Wc,128]; 8 [B,Hc,Wc,256];
 * 9 [B*Hc*Wc,65]; 10, 11 [B,Hc,Wc,256].                                                                                  */
int e2emv_superpoint_encode(e2emv_ctx* ctx, const e2emv_superpoint_desc* desc,
                            const float* d_images, /* [B,height,width] fp32, as for forward                                  */
                            float* d_score,        /* optional [B,H8,W8]: the map simple_nms receives                        */
                            float* d_dense,        /* optional [B,Hc,Wc,256] NHWC: the UNnormalised descriptor-head output   */
                            float* const* d_taps, void* stream);
/* The CONV mode of the fp32 GEMM alone, as e2emv_gemm_nt is its plain mode: a 3x3 / pad 1 / stride 1 convolution as an implicit
 * GEMM (rows = pixels, K = 9 * Cin, zero padding resolved in the operand fetch).  d_in [n_img,H,W,Cin] NHWC, d_w [Cout][9*Cin]
 * ordered (ky, kx, cin), d_bias [Cout] or NULL; flags: bit0 relu, bit1 the fused 2x2 / stride-2 max-pool (quad-major rows, maximum
 * taken in the epilogue); d_out [n_img,H,W,Cout], with the pool [n_img,H/2,W/2,Cout].  Cin % 32 == 0, n_img*H*W < 2^31, sides
 * <= 32767; the pool needs even sides, Cout % 4 == 0 and 16-byte aligned d_out / d_bias (E2EMV_ESHAPE otherwise); every pointer
 * 16-byte aligned.                                                                                                       */
int e2emv_conv3x3_nhwc(e2emv_ctx* ctx, int n_img, int H, int W, int Cin, int Cout, const float* d_in, const float* d_w,
                       const float* d_bias, int flags, float* d_out, void* stream);

/* ---- arithmetic of the dense GNN contractions -----------------------------------------
 * E2EMV_PRECISION_F32    : v_mfma_f32_32x32x2_f32, exact fp32 products (the audit mode).
 * E2EMV_PRECISION_BF16X3 : fp32 operands split into three bf16 planes, six bf16 MFMA products per
 *                          block accumulated in fp32 - fp32-class rounding (|err| ~ 2^-24 per
 *                          product) at 2.67x the fp32-MFMA ceiling.  Same API, same outputs within
 *                          the 1e-4 parity bar (tests/test_gpu_matcher.py runs every mode).
 * E2EMV_PRECISION_F16X2  : fp32 operands carried as two fp16 planes (hi + 2^-11 lo', 22 significant bits, the low plane
 *                          kept at the exponent range of the high one; static weights pre-scaled by a power of two per
 *                          matrix), three fp16 MFMA products per block accumulated in fp32: half the matrix-pipe work
 *                          of bf16x3.  Operand representation error <= 2^-22 for 6e-5 <= |x| <= 65504 (a K=512
 *                          contraction: 1e-7 rms, below fp32 accumulation noise); an activation beyond 65504 becomes
 *                          +-inf and surfaces as the sticky non-finite error of e2emv_sync.  DEFAULT.
 * Also selectable with the environment variable E2EMV_PRECISION=f32|bf16x3|f16x2 read at e2emv_create. */
#define E2EMV_PRECISION_F32 0
#define E2EMV_PRECISION_BF16X3 1
#define E2EMV_PRECISION_F16X2 2
int e2emv_set_precision(e2emv_ctx* ctx, int precision);
int e2emv_get_precision(e2emv_ctx* ctx, int* precision);
/* The split-operand modes use the fp32-MFMA kernels for calls with fewer than `min_rows` keypoint rows (images x
 * keypoints; default -1 = half a 128-row tile per CU, i.e. 16384 on an MI355X): their 64 x 64 tiles and key-split
 * attention are the latency-tuned forms for a pair or two.  0 = always the split kernels (how the parity tests reach
 * them at small sizes). */
int e2emv_set_split_min_rows(e2emv_ctx* ctx, int64_t min_rows);
/* building blocks of the bf16x3 path on fp32 buffers (split / merge done internally; for tests):
 * C = act(A W^T + bias), A [M,K], W [N,K], C [M,N] on gemm_x3.hip (fp32 activations split on the way into LDS); flags bit0
 * relu, bit2 = the f16x2 GEMM, gemm_h2.hip (host-synchronising: the weight planes are made on the host).  Bit1 (the retired
 * first-generation kernel on pre-split activation planes) returns E2EMV_EINVAL. */
int e2emv_gemm_bf16x3(e2emv_ctx* ctx, int M, int Nout, int K, const float* d_A, const float* d_W, const float* d_bias,
                      float* d_C, int flags, void* stream);
/* ... as the forward pass runs these kernels, with the argument list of e2emv_gemm_p2: C = act([A | A2] W^T + bias) (+ R);
 * A [M,K1], A2 [M,K-K1] or NULL (then K1 = K), W [N,K], R [M,N] or NULL; same flags.  e2emv_gemm_bf16x3 is this call with
 * K1 = K and no A2, no R. */
int e2emv_gemm_bf16x3_ex(e2emv_ctx* ctx, int M, int Nout, int K, int K1, const float* d_A, const float* d_A2, const float* d_W,
                         const float* d_bias, const float* d_R, float* d_C, int flags, void* stream);
/* same contract as e2emv_attention; cross: bit0 = cross layer, bit1 = the forward pass's kernel (fp32 q|k|v in, the
 * planes made inside the kernel) instead of the pre-split building block, bit2 = its f16x2 form. */
int e2emv_attention_bf16x3(e2emv_ctx* ctx, int B, int T, int n_rows, int n_valid, int D, int H, const float* d_qkv,
                           int cross, float* d_out, void* stream);
/* ... with a keypoint count per image of a tuple (HOST array of T ints; the contract of e2emv_attention_v) */
int e2emv_attention_bf16x3_v(e2emv_ctx* ctx, int B, int T, int n_rows, const int* n_valid_per_image, int D, int H,
                             const float* d_qkv, int cross, float* d_out, void* stream);

/* ---- f16x2 on plane activations (the default implementation of E2EMV_PRECISION_F16X2) ---------------------------
 * Activations live in HBM as the two fp16 planes of the f16x2 arithmetic (4 bytes per element like fp32, 32-column
 * blocks of {hi, lo}); every producer splits its output once in its epilogue, consumers move the planes from global
 * memory straight into LDS.  generation 5 (default) = these kernels (gemm_p2.hip; attention_p2w.hip - one wave per SIMD,
 * matrix and softmax work interleaved inside the wave - above 256 keys, attention_p2.hip below; needs descriptor_dim 256 /
 * 4 heads, other widths run the round-2 kernels that keep fp32 activations and split them inside the consuming GEMM /
 * attention) with the row-local GEMMs between two attentions (MLP0, MLP1, the next layer's q | k | v) chained per 256-row
 * block in ONE launch where that takes no more tile rounds than three launches (gemm_p2c.hip; bit-identical results; 105 =
 * chained on every shape that allows it), 4 = a launch per GEMM.  Other values (the retired generations 2 and 3 among
 * them) return E2EMV_EINVAL.  Also E2EMV_F16X2_KERNELS=r4 at e2emv_create (other values are ignored). */
int e2emv_set_f16x2_kernels(e2emv_ctx* ctx, int generation);
/* attention_p2w (f16x2, above 256 keys): when the (image, head, 256-query) items of a launch leave the last round of workgroups at most
 * half full - tuple_size 5 at 1024 keypoints: 640 items on 256 CUs, three rounds for 2.5 of work; a pair or two per call: fewer items
 * than CUs - the leftover items are split along the keys over the idle CUs and merged by a small second launch (on = 1, default; the
 * reference's shapes: eval_multi_view.py:154-162).  Results differ from the unsplit kernel by the order of the softmax sums only
 * (~1e-7 relative).  on = 0: never (A/B runs, tests). */
int e2emv_set_attention_key_split(e2emv_ctx* ctx, int on);
/* The front of the f16x2 plane forward - descriptor transpose, keypoint normalisation, the keypoint encoder and the conversion
 * of its output to planes - as ONE launch that keeps every intermediate on chip (kenc_fused.hip; on = 1, default) or as the
 * launch per stage it replaces (on = 0: A/B runs, tests).  The two compute the same bits.  The fused launch serves the plane
 * kernels with the keypoint encoder {3, 32, 64, 128, 256, 256}; every other call runs the stages whatever the switch says.
 * Also E2EMV_KENC=unfused at e2emv_create (other values are ignored). */
int e2emv_set_kenc_fused(e2emv_ctx* ctx, int on);
/* What that front hands to the GNN, for a call e2emv_matcher_forward would run on the plane kernels (else E2EMV_ESTATE): with
 * n_rows = N rounded up to 128 and M = B * T * n_rows, d_xp [M][2 * 256] halves = x as scaled planes (p2.h), d_ex [M / 64][4]
 * int32 = the tile exponents, d_ax [M / 64][4] f32 = the blocks' max |x|.  Honours e2emv_set_kenc_fused: a test compares the
 * two paths with it, without running a GNN.  Inputs as for e2emv_matcher_forward. */
int e2emv_encode_planes(e2emv_ctx* ctx, const e2emv_forward_desc* fd, const float* const* d_kpts, const float* const* d_kscores,
                        const void* const* d_desc, uint16_t* d_xp, int32_t* d_ex, float* d_ax, void* stream);
/* building blocks on fp32 buffers (conversion to / from planes done by helper kernels; for tests and micro-benchmarks):
 * C = act([A | A2] W^T + bias) (+ R); A [M,K1], A2 [M,K-K1] or NULL, W [N,K], R [M,N] or NULL.  flags: bit0 relu, bit1 the
 * kernel writes planes (converted back to fp32 afterwards) instead of fp32, bit2 = with the tile exponents of the range
 * side-band (M, K1, K - K1, N multiples of 64), bits 8.. = number of timed repetitions.  The
 * weight planes are made on the host as e2emv_commit_weights makes them (host-synchronising). */
int e2emv_gemm_p2(e2emv_ctx* ctx, int M, int Nout, int K, int K1, const float* d_A, const float* d_A2, const float* d_W,
                  const float* d_bias, const float* d_R, float* d_C, int flags, void* stream);
/* the q|k|v projection with its attention-operand epilogue (q | k planes + transposed V planes), read back as one fp32
 * matrix: d_X [n_img*n_rows, D], d_W [3D, D] head-major, d_qkv [n_img*n_rows, 3D]. */
int e2emv_qkv_p2(e2emv_ctx* ctx, int n_img, int n_rows, int D, int H, const float* d_X, const float* d_W, const float* d_bias,
                 float* d_qkv, void* stream);
/* same contract as e2emv_attention on the plane kernel; flags: bit0 cross, bit1 / bit2 force attention_p2 with 4 / 8 waves per workgroup, bit3 forces attention_p2w (one wave per SIMD),
 * bits 4..7 reserved (ignored), bits 8.. = timed repetitions. */
int e2emv_attention_p2(e2emv_ctx* ctx, int B, int T, int n_rows, int n_valid, int D, int H, const float* d_qkv, int flags,
                       float* d_out, void* stream);
/* ... with a keypoint count per image of a tuple (HOST array of T ints; the contract of e2emv_attention_v, except that
 * T > E2EMV_MAX_TUPLE is E2EMV_ESHAPE as in e2emv_attention_p2) */
int e2emv_attention_p2_v(e2emv_ctx* ctx, int B, int T, int n_rows, const int* n_valid_per_image, int D, int H,
                         const float* d_qkv, int flags, float* d_out, void* stream);

/* The matched descriptors of the LAST e2emv_matcher_forward call on this context (upstream's mdesc0 / mdesc1 = final_proj
 * output, models/superglue.py:269 upstream; with multi_frame_matching off and T > 2: of its last pair): d_out
 * [n_img = B*T][n_kpts][dim] fp32, keypoint-major.  d_out == NULL only reports the three sizes.  They live in the context's
 * workspace: any other call that uses the workspace (w8pt, BA, sinkhorn, superpoint, ...) ends their life, and a later
 * get_descriptors returns E2EMV_ESTATE instead of stale memory.  An audit output: the
 * quantity the arithmetic modes of the GNN differ in (tests/test_gpu_round4.py, tools/parity_margins.py). */
int e2emv_get_descriptors(e2emv_ctx* ctx, float* d_out, int64_t capacity_floats, int* n_img, int* n_kpts, int* dim, void* stream);

/* ---- range statistics ------------------------------------------------------------------------------------------------
 * The f16x2 mode keeps its fp16 planes inside fp16's range with one exponent per block of 64 x 64 activations (see
 * DESIGN.md 4d): there is no out-of-range fallback to take.  stats[0] = plane blocks that needed a non-zero exponent since
 * the last reset (0 for an ordinary network: every block sat inside the dead zone and took the plain paths), stats[1] =
 * Sinkhorn problems whose scores were non-finite (their outputs are NaN / inf and e2emv_sync reports them), stats[2] =
 * Sinkhorn problems the exponential-domain resident kernel could not finish (a scaling left fp32's range, or an
 * inter-workgroup wait gave up under contention) and the rescue pass behind it re-solved in the log domain inside the same
 * call: their outputs are correct, nothing is raised.  The host tells the two causes apart: the SECOND observation (here or
 * in e2emv_sync) of calls with range rescues moves the context to the log-domain launch chain - after 16 calls on it the
 * resident kernel gets another try -, rescues behind a timeout (stats[4] counts those) never do; stats[5] = Sinkhorn calls served by the 128-rows-per-workgroup
 * kernel (a batch of 513 .. 1024-column problems that it brings through in fewer rounds); stats[3] = (wave, stream, 64-key tile) softmaxes that
 * attention_p2w redid on its slow path (a performance counter: results are the same); stats[6] = launches of the fused
 * keypoint-encoder front (e2emv_set_kenc_fused).  Host-synchronising. */
int e2emv_get_stats(e2emv_ctx* ctx, uint64_t* stats, int n, int reset);

/* ---- which Sinkhorn kernel serves a call (upstream log_optimal_transport: models/superglue.py:156-186; reference call sites
 * /root/reference/helpers.py:246, eval_pairs.py:212) --------------------------------------------------------------------------
 * E2EMV_SINKHORN_AUTO (default): by shape AND batch size - the kernels with the couplings in registers addressed by number take
 * their full rounds, the remainder goes to the compiler-allocated kernel.  The kernels sum in different orders: a
 * problem's log-assignment can differ by < 2e-5 between two batch compositions.  ROWS64 / ROWS128 / ROWS128W pin one kernel kind
 * for every call of the context: a problem's result then does not depend on its batch neighbours, bit for bit.  At 513 .. 1024
 * columns there are two kernels of 128 rows per workgroup: ROWS128 = sinkhorn_resident128 (4 waves, couplings in vector and
 * accumulation registers), ROWS128W = sinkhorn_resident128w (8 waves, two per SIMD, vector registers only - the one AUTO takes);
 * elsewhere the two pins mean the same.  STREAM = the log-domain launch chain (no resident kernel; also taken for iters == 0).
 * The initial value comes from the environment variable E2EMV_SINKHORN = rows64 | rows128 | rows128w | stream, read ONCE at
 * e2emv_create. */
#define E2EMV_SINKHORN_AUTO 0
#define E2EMV_SINKHORN_ROWS64 1
#define E2EMV_SINKHORN_ROWS128 2
#define E2EMV_SINKHORN_STREAM 3
#define E2EMV_SINKHORN_ROWS128W 4
int e2emv_set_sinkhorn_kernel(e2emv_ctx* ctx, int kernel);
/* The launcher's plan for a batch of B problems of M x N scores and `iters` iterations on this context (what e2emv_sinkhorn /
 * e2emv_matcher_forward would launch now; nothing is launched): plan[0] = number of resident launches (0 = the log-domain chain, 1
 * or 2), then per launch 4 ints: rows of a problem per workgroup, problems of the batch it takes, problems resident at a time,
 * rounds.  n = capacity of plan (>= 9 for everything).  bench.py reports its Sinkhorn bound from this instead of re-deriving it. */
int e2emv_sinkhorn_plan(e2emv_ctx* ctx, int B, int M, int N, int iters, int* plan, int n);

/* ---- training: the matcher with a tape, the backward of the match loss and (through the confidences) of the pose loss ------
 * Replaces, for stage-1 training (match loss only), what torch.autograd does under the reference's
 *   pred = run_matcher(...); train_loss.backward()        (/root/reference/helpers.py:243-260, train.py:406-425)
 * with the reference's own arithmetic (fp32).  Differentiated: keypoint encoder, every GNN layer (projections, attention,
 * merge, MLP), final_proj, the score matrix, bin_score and the unrolled log-domain Sinkhorn (SuperGlue's
 * log_optimal_transport, models/superglue.py:156-186 upstream).  BatchNorm layers use their running statistics (frozen) or
 * the statistics of the batch (e2emv_train_set_batchnorm, below) and hand back gradients for their affine parameters either way.
 * The pose loss (helpers.py:253-258) reaches the network through the confidences: e2emv_w8pt_backward (below) ->
 * e2emv_conf_forward_train / d_dconf here.  Forward-only: images with differing keypoint counts, the confidences of a model
 * WITHOUT conf_mlp (the match score).
 *
 * e2emv_train_commit        folds the weights handed over with e2emv_set_weight into the training arena (call again after
 *                           every optimiser step, after re-sending the changed tensors).
 * e2emv_matcher_forward_train   same inputs as e2emv_matcher_forward (fd->n_kpts keypoints in every image); outputs the
 *                           log assignment matrices d_logZ[pair] = [batch][n_kpts + 1][n_kpts + 1] fp32, pairs in the
 *                           order (0,1), (0,2), (1,2), ... and keeps the tape of this call in the context.
 * e2emv_conf_forward_train  (models with conf_mlp; the pose loss) confidence head of one pair on the tape's matched descriptors:
 *                           d_conf [batch][n_kpts] = sigmoid(conf_mlp([mdesc_i[n] | mdesc_j[match n]])) for matched n, else 0;
 *                           d_matches0 = that pair's matches (e.g. from e2emv_extract_matches on d_logZ), kept alive by the
 *                           caller until the backward.
 * e2emv_matcher_backward    d_dlogZ[pair] = dLoss / dlogZ of the last forward_train (same layout; a null entry = zero),
 *                           d_dconf (may be null) [pair] = dLoss / dconf of e2emv_conf_forward_train (a null entry = zero):
 *                           leaves the gradient of every upstream parameter in the context.
 * e2emv_get_grad            copies the gradient of parameter `key` (the reference's state_dict name, an optional "module."
 *                           prefix is ignored) into d_dst (device, fp32, numel elements); stream-ordered.                 */
int e2emv_train_commit(e2emv_ctx* ctx, const e2emv_model_desc* model);
/* After an optimiser step (helpers.py / train.py: optimizer.step() between two forwards): the new values of the model's
 * floating-point state_dict tensors straight from DEVICE memory (d_params[i] = fp32, contiguous, numels[i] elements, name
 * keys[i]; tensors the differentiable path does not use are ignored) into the training arena that e2emv_train_commit built for
 * this model - device-to-device copies and the BatchNorm / head-order folds as kernels, stream-ordered, no host copy and no
 * synchronisation.  bin_score = the scalar parameter's value.  E2EMV_ESTATE when the context holds no arena of this model
 * (then: e2emv_set_weight for every tensor + e2emv_train_commit, once).  The host-side weight store of e2emv_set_weight is
 * NOT updated: hand the tensors over again before the next e2emv_commit_weights.                                          */
int e2emv_train_update(e2emv_ctx* ctx, const e2emv_model_desc* model, int n, const char* const* keys, const float* const* d_params,
                       const int64_t* numels, float bin_score, void* stream);
int e2emv_matcher_forward_train(e2emv_ctx* ctx, const e2emv_forward_desc* fd, const float* const* d_kpts, const float* const* d_kscores,
                                const void* const* d_desc, float* const* d_logZ, void* stream);
int e2emv_conf_forward_train(e2emv_ctx* ctx, int pair, const int64_t* d_matches0, float* d_conf, void* stream);
int e2emv_matcher_backward(e2emv_ctx* ctx, const float* const* d_dlogZ, const float* const* d_dconf, void* stream);
int e2emv_get_grad(e2emv_ctx* ctx, const char* key, float* d_dst, int64_t numel, void* stream);
/* BatchNorm of the training path.  E2EMV_BN_FROZEN (the default): every BatchNorm normalises with its running statistics,
 * folded into the convolution in front of it, and the buffers are not written.  E2EMV_BN_BATCH: torch's BatchNorm1d in
 * training mode (the reference's matcher.train(), train.py:348) - each call normalises with the statistics of its own rows
 * (biased variance, eps 1e-5) and the backward is the batch-statistics gradient.  One call per image for kenc.encoder.{1,4,..}
 * and gnn.layers.{l}.mlp.1 (t = 0 .. T-1 in order), one per pair for conf_mlp.1 (its B x n_kpts features, unmatched rows
 * included); padding rows never enter a sum; statistics are fp64 partials combined in a fixed order (bitwise reproducible).
 *
 * e2emv_train_set_batchnorm   selects the mode and the momentum of the running update (one value for every BatchNorm).  A mode
 *                             other than the arena's makes e2emv_train_update and e2emv_matcher_forward_train return
 *                             E2EMV_ESTATE: hand the tensors over again and e2emv_train_commit.
 * e2emv_train_running_update  (E2EMV_BN_BATCH) applies the statistics of the last forward_train and of its conf forwards (each
 *                             pair whose conf head ran, in pair order) to the caller's buffers, call by call:
 *                               mean <- (1 - m) mean + m mean_call,  var <- (1 - m) var + m var_call n / (n - 1),  n = batch x n_kpts
 *                             keys[i] = BatchNorm module name (e.g. "gnn.layers.3.mlp.1", an optional "module." prefix is
 *                             ignored), d_running_mean[i] / d_running_var[i] = its fp32 device buffers.  Stream-ordered, no
 *                             synchronisation; num_batches_tracked is the caller's (+ T, or + the conf calls).  E2EMV_ESTATE
 *                             without a tape or in frozen mode.
 * Not covered: momentum None (cumulative average), SyncBatchNorm across ranks, .train() without gradients (the inference
 * path, running statistics).                                                                                              */
#define E2EMV_BN_FROZEN 0
#define E2EMV_BN_BATCH 1
int e2emv_train_set_batchnorm(e2emv_ctx* ctx, int mode, float momentum);
int e2emv_train_running_update(e2emv_ctx* ctx, int n, const char* const* keys, float* const* d_running_mean, float* const* d_running_var,
                               void* stream);

/* Backward of e2emv_w8pt with respect to the confidences (training, the pose loss of helpers.py:253-258: rot / translation
 * error of run_weighted_8_point's pose).  Inputs: the normalised correspondences and the pose the forward returned (info
 * "kpts0_norm" / "kpts1_norm", T), the confidences it was given, d_gT = dLoss/dT [B][4][4]; output d_gconf [B][N].  The
 * derivative of the eigenvector is analytic, the 9 -> 12 Jacobian of the rank-2 / decomposition tail is taken by central
 * differences in fp64.  The candidate choice (choose_closest / cheirality) is piecewise constant: the candidate the forward
 * chose is differentiated. */
int e2emv_w8pt_backward(e2emv_ctx* ctx, int B, int N, const float* d_kpts0n, const float* d_kpts1n, const float* d_conf, const float* d_T,
                        const float* d_gT, float* d_gconf, void* stream);

/* Backward of e2emv_pose_errors with respect to d_T (compute_rotation_error / compute_translation_error_as_angle as the pose
 * loss, helpers.py:256-258): d_gT [B][4][4] = d_g_rot[b] d rot_b / dT + d_g_transl[b] d transl_b / dT. */
int e2emv_pose_errors_backward(e2emv_ctx* ctx, int B, const float* d_T, const float* d_T_gt, const float* d_g_rot, const float* d_g_transl,
                               float* d_gT, void* stream);

/* Backward of e2emv_w8pt_tuple with respect to the P = T(T-1)/2 confidence tensors, in the forward's pair order and pair-major
 * indexing.  d_matches[q] / d_conf[q] [B,N]: the forward's inputs; d_kpts0n / d_kpts1n [P*B,N,2] and d_T [P*B,4,4]: its outputs;
 * d_gT [P*B,4,4] = dLoss/dT.  Element (q, b) is e2emv_w8pt_backward for the confidences the forward's solve saw,
 * c = matches >= 0 ? conf : 0; d_gcf [P*B,N] (may be NULL), the adjoint of those gathered confidences themselves, is added to its
 * result g, and d_gconf[q][b,n] = matches >= 0 ? g : 0.  A NULL d_gconf[q] leaves that pair out.  One gather, the backward kernel
 * of e2emv_w8pt_backward on all P*B samples, one masked scatter.  Errors as e2emv_w8pt_tuple: E2EMV_ESHAPE for B <= 0, T outside
 * 2..E2EMV_MAX_TUPLE or N < 8, E2EMV_EINVAL for a NULL table or a NULL entry of d_matches / d_conf; nothing is launched then. */
int e2emv_w8pt_tuple_backward(e2emv_ctx* ctx, int B, int T, int N, const int64_t* const* d_matches, const float* const* d_conf,
                              const float* d_kpts0n, const float* d_kpts1n, const float* d_T, const float* d_gT, const float* d_gcf,
                              float* const* d_gconf, void* stream);

/* The pose term of helpers.run_matcher (helpers.py:250-258) for the P pairs of a tuple batch, reduced on the device: d_T / d_T_gt
 * [P*B,4,4] pair-major; per-element errors and validity [P*B] as e2emv_pose_error_means; d_losses2[0] = sum over q of the mean
 * rotation error of pair q over its B entries, d_losses2[1] = sum over q of the mean translation error over the valid entries of
 * pair q (NaN for a pair with none, which makes the sum NaN like the reference's mean of an empty selection).  Each mean with the
 * arithmetic of e2emv_pose_error_means, the pairs added in fp32 in ascending q. */
int e2emv_pose_loss_tuple(e2emv_ctx* ctx, int P, int B, const float* d_T, const float* d_T_gt, float* d_rot_err, float* d_transl_err,
                          uint8_t* d_transl_valid, float* d_losses2, void* stream);

/* Backward of e2emv_pose_loss_tuple with respect to d_T: d_g2 = DEVICE pointer to {dL/d losses2[0], dL/d losses2[1]}; d_gT [P*B,4,4]
 * is e2emv_pose_errors_backward with g_rot[q,b] = g2[0] / (float)B and g_transl[q,b] = valid ? g2[1] / (float)n_valid_q : 0, both
 * formed in fp32 on the device (no host synchronisation). */
int e2emv_pose_loss_tuple_backward(e2emv_ctx* ctx, int P, int B, const float* d_T, const float* d_T_gt, const float* d_g2, float* d_gT,
                                   void* stream);

/* ---- the match term of a training step for all pairs of a tuple (helpers.run_matcher, helpers.py:243-253) ----
 * Pair order as everywhere: q counts (i, j) for j in range(T): for i in range(j); P = T(T-1)/2; pair-major buffers [P,B,...].
 *
 * e2emv_gt_matches of every pair of B tuples of T images in one call: d_kpts / d_K / d_pose / d_depth are HOST arrays of T DEVICE
 * pointers (image t: [B,N,2], [B,4,4], [B,4,4] = data["pose t"], [B,H,W]).  The relative pose of pair (i, j), inv(pose_j) @ pose_i,
 * is formed on the device with the arithmetic of e2emv_relative_pose and rounded to fp32 as that entry stores it; the three
 * kernels of e2emv_gt_matches then run with the pair as one more grid dimension.  d_indices [P,B,2,N+1] int64 and d_weights
 * [P,B,2,N+1] fp32 are, bit for bit, the stacked outputs of e2emv_relative_pose + e2emv_gt_matches per pair.  Four launches
 * whatever P and B, no host synchronisation.  E2EMV_ESHAPE: T outside 2..E2EMV_MAX_TUPLE or B, N, H, W <= 0; E2EMV_EINVAL: a NULL
 * context, table, table entry or output; nothing is launched then. */
int e2emv_gt_matches_tuple(e2emv_ctx* ctx, int B, int T, int N, const float* const* d_kpts, const float* const* d_K,
                           const float* const* d_pose, const float* const* d_depth, int H, int W, float max_matched_reproj_err,
                           float min_unmatched_reproj_err, int64_t* d_indices, float* d_weights, void* stream);

/* d_logZ = HOST array of P DEVICE pointers [B,N+1,N+1]; d_indices / d_weights [P,B,2,N+1] as above.  The loss of pair q is
 * e2emv_match_loss to the bit (fp64 partial sums per batch element, folded in ascending b, divided by B, cast to fp32) and goes
 * to d_pair_loss[q] (DEVICE, [P], may be NULL); d_loss[0] is their fp32 sum in ascending q starting from 0.0f, the order of
 * `match_loss = match_loss + ...`.  Two launches.  E2EMV_ESHAPE: P outside 1..28 or B, N <= 0. */
int e2emv_match_loss_tuple(e2emv_ctx* ctx, int P, int B, int N, const float* const* d_logZ, const int64_t* d_indices,
                           const float* d_weights, float* d_loss, float* d_pair_loss, void* stream);

/* Backward of e2emv_match_loss_tuple to the scores, one launch that does not read them: d_g = DEVICE pointer to dL/d loss;
 * d_glogZ = HOST array of P DEVICE pointers [B,N+1,N+1] (4-byte alignment suffices; a NULL entry leaves that pair out).  With
 * ft = N+1, gb = g / (float)B in fp32, col0(r) = idx0[r] < 0 ? idx0[r] + ft : idx0[r] and row1(c) likewise from idx1[c]:
 *   d_glogZ[q][b][r][c] = (c == col0(r) ? -(gb * w0[r]) : 0) + (r == row1(c) ? -(gb * w1[c]) : 0)
 * EVERY element is written (the buffers may hold anything on entry; no memset, no atomics); an index outside [-ft, ft) contributes
 * nothing.  E2EMV_ESHAPE: P outside 1..28, B outside 1..16383, N outside 1..46338. */
int e2emv_match_loss_tuple_backward(e2emv_ctx* ctx, int P, int B, int N, const int64_t* d_indices, const float* d_weights,
                                    const float* d_g, float* const* d_glogZ, void* stream);

/* ---- the optimiser step of the training loop (train.py:419-426: has_finite_gradients, clip_grad_value_, Adam.step) -------------
 * All parameter tensors of a call in at most three launches and one memset, stream-ordered, no host synchronisation.  The tensor
 * table and chunk list of a call live in a buffer the context keeps for them (not the shared workspace) and are uploaded only
 * when they differ from the previous call's (such a call waits for the copy of the previous table, long done, to leave the pinned
 * staging buffer, and a call with a larger table than any before allocates; a call with the same pointers does neither). */
#define E2EMV_OPTIM_CHUNK 4096   /* elements one workgroup handles at a time; a chunk never crosses a tensor */

/* *d_flag (device int32) = 1 if any element of any of the n tensors is NaN or +-inf, else 0.  Host arrays of n device
 * pointers / element counts; stream-ordered, no synchronisation.  n == 0: flag = 0.  A tensor with numel == 0 is skipped.
 * E2EMV_EINVAL: NULL context, array, entry (of a tensor that has elements) or flag; E2EMV_ESHAPE: n < 0, a negative numel, more chunks than an int counts. */
int e2emv_grads_finite(e2emv_ctx* ctx, int n, const float* const* d_grad, const int64_t* numel, int32_t* d_flag, void* stream);

/* One Adam step (torch.optim.Adam: no weight decay, no amsgrad, not maximising) for n tensors in place.
 * d_step[i]: device float32 scalar, the number of steps tensor i has taken (torch's capturable layout).
 * lr[i]: host, per tensor.  clip_value > 0: the gradient is clamped to [-clip_value, clip_value] first (clip_grad_value_); <= 0: no clip.
 * skip_nonfinite != 0: if any gradient element of the CALL is non-finite, nothing is written - no parameter, moment or step
 * changes by a bit - and d_counters[1] += 1; otherwise every tensor is updated, d_step[i] += 1, d_counters[0] += 1.
 * skip_nonfinite == 0: always updated (a NaN gradient reaches its own element, as in torch).  d_counters: device int32 [2] or NULL.
 * Per element, fp32, with t = step + 1:  g = clamp(g);  m += (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g^2;
 * p -= (lr / (1 - beta1^t)) * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps)) - the two bias corrections in fp64 from the device's
 * step value.  Errors as above, nothing launched. */
int e2emv_adam_step(e2emv_ctx* ctx, int n, float* const* d_param, const float* const* d_grad, float* const* d_exp_avg,
                    float* const* d_exp_avg_sq, float* const* d_step, const int64_t* numel, const float* lr,
                    double beta1, double beta2, double eps, float clip_value, int skip_nonfinite, int32_t* d_counters, void* stream);

/* ---- the image front of a tuple (MatchingDataset.__getitem__, datasets/matching_dataset.py:182-211) -------------
 * ToTensor (u8 / 255, a true fp32 division), ONE source window, the bilinear resize, ColorJitter with one parameter row per
 * image and rgb_to_grayscale: d_rgb uint8 [B][in_height][in_width][3] (interleaved, what a JPEG decoder hands out) ->
 * d_gray float32 [B][1][out_height][out_width], the tensor e2emv_superpoint_forward takes.
 * Window: the rectangle (win_top, win_left, win_height, win_width) in source coordinates; it may reach outside the image, where
 * it reads zeros - the 2-row padding of the large ScanNet frames is win_top = -2, win_height = in_height + 4, the square crop
 * of MegaDepth a window inside the image.  The window is resized to the output size with the semantics of
 * torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=antialias) (tap tables in fp64 on the host,
 * once per shape); a window of the output's size is copied, no arithmetic touches the values.
 * LIMIT: the source columns that E2EMV_IMAGE_FRONT_TILE neighbouring output columns need (about 64 * scale + 2 * scale + 1 with
 * antialias, 64 * scale + 2 without) must not exceed E2EMV_IMAGE_FRONT_STRIP - a horizontal down-scale up to about 5.8;
 * E2EMV_ESHAPE beyond it.  The vertical scale is not limited.
 * Jitter: order / factors are HOST arrays [B][4] (both or neither; NULL = no jitter): order[b][slot] names the op of the slot
 * (0 brightness, 1 contrast, 2 saturation, 3 hue, -1 = the slot is skipped), factors[b] = (brightness, contrast, saturation,
 * hue).  The ops are torchvision's tensor forms on values in [0, 1]; the contrast blend takes the mean gray value of the whole
 * image as it stands at that slot (a fixed-order two-stage sum: the same call gives the same bytes every time).
 * d_rgb_out: optional [B][3][out_height][out_width], the jittered colour image the gray value is taken of (audits); may be NULL.
 * Launches: one when no image of the call has a contrast slot, else three (the resample with the partial sums, the means,
 * the jitter); stream-ordered, no host synchronisation; tap tables, the workspaces of a call with a contrast slot (one partial
 * sum per tile and the resized colour image as fp32, 12 bytes per output pixel of the call; E2EMV_ENOMEM if they cannot be
 * reserved) and the parameter rows live in the context - nothing is allocated after the first call of a shape.  The
 * parameter rows (48 bytes per image) are copied from a pinned ring of the context.
 * E2EMV_EINVAL, with a message and nothing launched: a NULL context, descriptor, d_rgb or d_gray; order without factors or the
 * reverse; a non-positive size; an empty window; antialias other than 0 | 1; an order entry outside -1..3 or an op named twice;
 * a factor that is not finite; a negative brightness, contrast or saturation factor; a hue factor outside [-0.5, 0.5]. */
#define E2EMV_IMAGE_FRONT_TILE 64    /* output columns of a tile (its rows: 16) */
#define E2EMV_IMAGE_FRONT_STRIP 384  /* source columns a tile may span */
typedef struct {
    int32_t batch;                  /* B                                              */
    int32_t in_height, in_width;    /* Hin, Win                                       */
    int32_t win_top, win_left;      /* the window's first row / column, may be < 0    */
    int32_t win_height, win_width;  /* > 0; may reach beyond the image                */
    int32_t out_height, out_width;  /* Hout, Wout                                     */
    int32_t antialias;              /* 0 | 1                                          */
} e2emv_image_front_desc;
int e2emv_image_front(e2emv_ctx* ctx, const e2emv_image_front_desc* desc, const uint8_t* d_rgb, const int32_t* order,
                      const float* factors, float* d_gray, float* d_rgb_out, void* stream);

/* ---- the image front of pair evaluation (PairMatchingDataset.__getitem__, eval_pairs.py:85-108) -------------
 * Per image: the decoded gray frame, uint8 [height][width] on the device (cv2.imread(.., IMREAD_GRAYSCALE)), is turned by
 * `rot` quarter turns counter-clockwise (np.rot90(img, k=rot); the turned image is never made, the turn is part of the source
 * addressing), resized so that its longer side is img_size (e2emv_image_front_gray_size; no resize when it already is) and
 * divided by 255: float32 [h_out][w_out], what e2emv_superpoint_forward takes.  images: a HOST array of n records; d_out: ONE
 * device buffer in which image i's h_out_i * w_out_i floats follow image i - 1's.  The images of a call may all differ in
 * size and turn.
 * Resize: cv2.resize's INTER_LINEAR on a float32 image - two taps per axis, half-pixel centres, no antialiasing; per axis, with
 * scale = 1.0 / (double(n_out) / double(n_in)), output index d reads f = float32((d + 0.5) * scale - 0.5) (the product and the
 * difference in double, one rounding to float32), s = floor(f), f -= s; s < 0: s = 0, f = 0; s >= n_in - 1: s = n_in - 1, f = 0;
 * weights (float32(1) - f, f) on the pixels s and min(s + 1, n_in - 1); the horizontal taps first, on the values 0..255, then
 * the vertical ones, then the fp32 division by 255.  The tap positions are computed in the kernel, in exactly this arithmetic.
 * An image that is not resized is u8 / 255 with the bytes of the true fp32 division.
 * One launch per call whatever n and the sizes are; stream-ordered, no host synchronisation; no atomics: the same call gives
 * the same bytes.  The table of the call (64 bytes per image) is copied from a pinned ring of the context; everything the call
 * needs is reserved by the first call of a context.
 * LIMITS (E2EMV_ESHAPE with a message, nothing launched): a side of a frame, or img_size, above 16384; an image whose tiles need
 * more of the source than the 24 KB a workgroup stages: a tile of E2EMV_IMAGE_FRONT_GRAY_TILE_ROWS x _TILE_COLS output pixels
 * keeps at most 64 source lines of (32 * scale + 2) bytes (+ up to 30 of alignment) - a reduction up to about 10 on either
 * axis, 8 guaranteed; enlargements are not limited.
 * E2EMV_EINVAL, with a message and nothing launched: a NULL context, images, d_out or frame pointer; n <= 0 or n above
 * E2EMV_IMAGE_FRONT_GRAY_MAX_IMAGES; a non-positive height, width or img_size; rot outside 0..3; an output side that truncates to 0.
 * e2emv_image_front_gray_size: host only - the output size of a stored height x width frame turned by rot, in the reference's
 * own arithmetic (eval_pairs.py:96-102): the turned image h x w is kept when img_size == max(h, w); else, h >= w:
 * (img_size, int((w / h) * img_size)), otherwise (int((h / w) * img_size), img_size) - Python's doubles and truncation, not an
 * integer division (10 x 7 at 720: 503 columns).  E2EMV_EINVAL for the arguments named above. */
#define E2EMV_IMAGE_FRONT_GRAY_TILE_ROWS 32    /* output rows of a tile */
#define E2EMV_IMAGE_FRONT_GRAY_TILE_COLS 32    /* output columns of a tile */
#define E2EMV_IMAGE_FRONT_GRAY_MAX_IMAGES 256  /* images of one call */
typedef struct {
    const uint8_t* data;    /* device, [height][width], rows contiguous, any alignment */
    int32_t height, width;  /* as stored (before the turn)                             */
    int32_t rot;            /* 0..3 quarter turns counter-clockwise                    */
} e2emv_gray_image;
int e2emv_image_front_gray_size(int height, int width, int rot, int img_size, int* h_out, int* w_out);
int e2emv_image_front_gray(e2emv_ctx* ctx, int n, const e2emv_gray_image* images, int img_size, float* d_out, void* stream);

/* ---- timing hooks used by bench.py (HIP events on the caller's stream) -------------
 * After e2emv_profile(ctx, 1) every kernel family launched by the library is bracketed by
 * HIP events on its stream; e2emv_profile_read returns accumulated milliseconds and launch
 * counts per family since the last reset (host-synchronising).                             */
#define E2EMV_PROF_SLOTS 16
int e2emv_profile(e2emv_ctx* ctx, int enable);
int e2emv_profile_read(e2emv_ctx* ctx, float* ms, int64_t* launches, int n_slots, int reset);
const char* e2emv_profile_name(int slot);

/* ---- the one collective of the path: metric gather / reduction over the ranks of a node (RCCL over xGMI) --------------------------
 * Replaces, for a host without torch.distributed, the reference's init_process_group(backend="nccl") (/root/reference/train.py:
 * 270-277) and its only explicit collective, the all_reduce of the validation loss (train.py:102-106); the evaluation scripts'
 * per-pair pose errors are gathered with the same communicator for the exact sort-based AUC.  One process per GPU; tuples are
 * sharded, the data path has no collective.  librccl.so.1 is dlopen'ed by the first of these calls (E2EMV_ESTATE if absent).
 *   rank 0: e2emv_comm_unique_id -> hand the 128 bytes to every rank (file, environment, the launcher's store) ->
 *   every rank: e2emv_comm_init (collective: returns when all `world` ranks called it) -> e2emv_metric_* -> e2emv_comm_destroy.
 * e2emv_comm_init_file does the hand-over through a file all ranks see (rank 0 writes path atomically, the others poll up to
 * timeout_s seconds).  d_* buffers are device memory of the context's device; calls are ordered on `stream`. */
#define E2EMV_COMM_ID_BYTES 128
typedef struct e2emv_comm e2emv_comm;
int e2emv_comm_unique_id(e2emv_ctx* ctx, void* id_out /* [E2EMV_COMM_ID_BYTES] */);
int e2emv_comm_init(e2emv_ctx* ctx, const void* id, int rank, int world, e2emv_comm** out);
int e2emv_comm_init_file(e2emv_ctx* ctx, const char* path, int rank, int world, double timeout_s, e2emv_comm** out);
int e2emv_comm_destroy(e2emv_ctx* ctx, e2emv_comm* comm);
int e2emv_comm_rank(const e2emv_comm* comm, int* rank, int* world);
/* d_all [world][n] <- every rank's d_local [n], rank order, on every rank */
int e2emv_metric_allgather(e2emv_ctx* ctx, e2emv_comm* comm, const float* d_local, int n, float* d_all, void* stream);
/* d_buf [n] <- op over the ranks, in place */
#define E2EMV_REDUCE_SUM 0
#define E2EMV_REDUCE_MAX 1
#define E2EMV_REDUCE_MIN 2
int e2emv_metric_allreduce(e2emv_ctx* ctx, e2emv_comm* comm, float* d_buf, int n, int op, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* E2EMV_H */
