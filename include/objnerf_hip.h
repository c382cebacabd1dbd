/*
 * objnerf_hip.h -- C ABI of libobjnerf_hip.so, the MI355X (gfx950) implementation of OpenObj's
 * vectorised object-NeRF hot path.
 *
 * The reference (BIT-DYN/OpenObj, objnerf/) has no FFI / operator layer of its own: its hot path
 * is a Python call sequence (train.py:394-474).  This header is the boundary a maintainer binds
 * that call sequence to; each entry point cites the reference interface it replaces.  All
 * pointers are DEVICE pointers unless named host_*; all tensors are contiguous row-major fp32
 * unless stated; outputs and workspaces are caller-allocated; nothing here allocates, frees or
 * synchronises, and every launch goes to `stream` (a hipStream_t passed as void*) -- with ONE explicit
 * exception: an objnerf_context (below) holds helper streams and events the caller creates and hands to
 * objnerf_train_step so that the layer-wise path can run independent GEMMs side by side; its work is
 * forked from and joined back into `stream` with events, so `stream` order still describes completion.
 * Kernel attributes (the opt-in to > 64 KB LDS) are set once per device, thread-safely, at first use.  Return value:
 * 0 on success, a negative OBJNERF_E* code otherwise (the reference's assert / exit(-1) paths).
 *
 * Symbols (paths relative to the reference's objnerf/):
 *   K objects, R rays per object, S samples per ray, H hidden width, C feature width (512),
 *   E1=87 / E2=42 embedding split (trainer.py:20-21).
 *
 * Parameter arena.  The reference stacks the K networks into 18+1 tensors with
 * functorch.combine_state_for_ensemble (utils.py:55-62).  Here the same values live in ONE
 * object-major fp32 arena [K][P_stride]: object k's 19 tensors back to back in the order of
 * OccupancyMap.parameters() (model.py:29-56) followed by UniDirsEmbed.B_layer.weight
 * (embedding.py:39-40).  objnerf_param_layout() returns the offsets; the stacked tensors the
 * reference API exposes are strided views of the arena.  Gradients and Adam moments use the same
 * layout.
 */
#ifndef OBJNERF_HIP_H
#define OBJNERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OBJNERF_ABI_VERSION 14

#define OBJNERF_OK 0
#define OBJNERF_EINVAL (-22)       /* bad shape / null pointer / unsupported size        */
#define OBJNERF_ENOTSUP (-95)      /* shape valid for the reference but not built here   */
#define OBJNERF_ELAUNCH (-5)       /* HIP launch error (hipGetLastError != hipSuccess)   */

#define OBJNERF_N_TENSORS 19       /* 18 OccupancyMap tensors + B_layer.weight           */

/* Index of each tensor inside an object's block of the arena (model.py:29-56 order). */
enum objnerf_tensor {
  OBJNERF_T_IN_W = 0, OBJNERF_T_IN_B, OBJNERF_T_M1_W, OBJNERF_T_M1_B, OBJNERF_T_CAT_W,
  OBJNERF_T_CAT_B, OBJNERF_T_M2_W, OBJNERF_T_M2_B, OBJNERF_T_ALPHA_W, OBJNERF_T_ALPHA_B,
  OBJNERF_T_CL_W, OBJNERF_T_CL_B, OBJNERF_T_OC_W, OBJNERF_T_OC_B, OBJNERF_T_FL_W, OBJNERF_T_FL_B,
  OBJNERF_T_OF_W, OBJNERF_T_OF_B, OBJNERF_T_PE_B
};

/* Network shape: trainer.py:15-21,36-44. */
typedef struct objnerf_net {
  int32_t hidden;        /* cfg.hidden_feature_size (32 objects / 128 background)         */
  int32_t feat_dim;      /* cfg.clip_point_feature_size (512)                             */
  int32_t n_freqs;       /* cfg.n_unidir_funcs + 1 (6)                                    */
  int32_t reserved;
} objnerf_net;

/* offsets[i] = start of tensor i inside an object's block, offsets[19] = parameter count P;
 * returns P_stride (P rounded up to 64 floats), or a negative error. */
int64_t objnerf_param_layout(const objnerf_net* net, int64_t offsets[OBJNERF_N_TENSORS + 1]);

int objnerf_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * A1  cameraInfo.get_rays_dirs (vmap.py:701-720): out [W][H][3], un-normalised, transposed image.
 */
int objnerf_rays_dirs(int32_t W, int32_t H, float fx, float fy, float cx, float cy, float* out,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * A2+A3+A4  sceneObject.get_training_samples + sample_3d_points (vmap.py:386-554,
 * utils.py:324-397) for ONE object: gather pixels from the keyframe buffers and place the
 * depth-guided z-values.
 * Randomness, INJECTED form (exact parity with the reference's torch.rand / normal_ draws):
 *   kf_ids [n_frames] int64, u_w,u_h [n_frames][n_px] in [0,1),
 *   u [n_frames*n_px][N+M] uniforms, g [n_frames*n_px][M] draws of N(0,(eps/3)^2).
 * Randomness, SEEDED form (u_w = u_h = u = g = NULL): every draw is Philox4x32-10 of
 *   (seed; purpose, draw; object index, ray, bin) computed in place -- no random number is ever stored.  `draw` is
 *   the caller's call counter (a new value = new draws, 29 bits), the object index identifies the object's random
 *   stream (kf_meta[3]; without kf_meta: obj_index, + k for object k of a stacked call), so that objects,
 *   iterations and GPUs holding different objects never share a draw.
 *   kf_ids may then be NULL too: kf_meta [4] int32 = {n_keyframes, slot of the second-latest keyframe, slot of the
 *   latest (-1, -1 while n_keyframes <= 2), object index} selects the keyframes as vmap.py:390-401 does (uniform
 *   over the stored keyframes, the latest two always included, LAST).  out_kf [n_frames] int64 / out_px [n][2] int32 (pixel
 *   (w, h) of each ray) are optional records of what was drawn (the part-feature gather of vmap.py:437-452 needs
 *   them).
 * Keyframe buffers: rgbs [F][W][H][4] u8 (rgb+state), depth [F][W][H], t_wc [F][4][4],
 * bbox [F][4] = [u lo,u hi,v lo,v hi], rays_dir_cache [W][H][3].
 * Outputs: rgb [n][3] u8, gt_depth [n], valid [n] u8, labels [n] u8, z [n][N+M], pts [n][N+M][3]
 * (n = n_frames*n_px).  out_pts may be NULL when out_origins / out_dirs [n][3] are given: the world-frame ray
 * origins and directions go there and objnerf_train_step (pts == NULL form) forms the points in registers --
 * the [n][N+M][3] point tensor is then never written or read.
 * max_depth_ws: device scratch of 1 + 6*n floats ([0] receives the batch depth
 * maximum of vmap.py:489, the rest holds the world-frame origins / directions between the passes).
 */
typedef struct objnerf_sample_args {
  int32_t F, W, H, n_frames, n_px, n_cam2surf, n_bins, obj_index;
  float surface_eps, stop_eps, min_bound, obj_center;
  const uint8_t* rgbs; const float* depth; const float* t_wc; const float* bbox;
  const float* rays_dir_cache;
  const int64_t* kf_ids; const float* u_w; const float* u_h; const float* u; const float* g;
  uint8_t* out_rgb; float* out_depth; uint8_t* out_valid; uint8_t* out_labels;
  float* out_z; float* out_pts; float* max_depth_ws;
  /* ABI 3 */
  uint64_t seed; uint32_t draw; uint32_t reserved;
  const int32_t* kf_meta; int64_t* out_kf; int32_t* out_px;
  float* out_origins; float* out_dirs;
  /* ABI 6 -- the part-level feature gather of vmap.py:437-452 inside the same launch (out_partfeat == NULL: off).
   * global_partfeat [pf_frames][pf_w][pf_h][pf_c] fp32: the scene's part-feature maps (train.py:378), one per used
   * dataset frame; use_frame [F] int32: dataset frame id of every keyframe slot (vmap.py:108,199-231; stacked call:
   * [K][F]); the ray's source row is frame trunc(use_frame[kf] / pf_stride) (float64 quotient, :440), pixel
   * (floor(idx_w / part_down), floor(idx_h / part_down)) with the FLOAT pixel index divided in fp32 (:441-442).
   * out_partfeat [n][pf_c] (stacked: [K][n][pf_c]) is written once, a wave per ray, 16-byte lanes.  Indices outside
   * the map are clamped (the reference raises IndexError; the host wrapper checks the frame range). */
  const float* global_partfeat; const int32_t* use_frame; float* out_partfeat;
  int32_t pf_frames, pf_w, pf_h, pf_c, pf_stride; float part_down;
  /* ABI 12 -- the same gather through an index image (part_index == NULL: the dense form above, unchanged).
   * part_index [pf_frames][pf_w][pf_h] int32 holds, for the pixel the dense form would read, a row number of
   * global_partfeat, which is then the row TABLE [pf_rows][pf_c] (row 0 = zeros: a pixel no mask covers); frame and
   * pixel are computed as above, the row number is clamped to [0, pf_rows). */
  const int32_t* part_index; int32_t pf_rows; int32_t reserved_pf;
} objnerf_sample_args;
int objnerf_sample_rays(const objnerf_sample_args* a, void* stream);

/* The same for K objects in ONE launch chain (train.py:316-330 calls the sampler once per object and stacks the
 * results, train.py:368-388).  `table`: DEVICE array of K keyframe-store descriptors (the objects share F, W, H and
 * every scalar of `a`; a->rgbs / depth / t_wc / bbox are ignored).  Every draw and output array of `a` (kf_meta,
 * out_kf, out_px, out_origins, out_dirs included) is stacked [K][...] with the per-object layouts above -- the outputs ARE the stacked batch tensors of the training step --
 * and max_depth_ws holds K x (1 + 6 n) floats. */
typedef struct objnerf_kf_store {
  const uint8_t* rgbs; const float* depth; const float* t_wc; const float* bbox;
} objnerf_kf_store;
int objnerf_sample_rays_stacked(const objnerf_sample_args* a, int32_t K, const objnerf_kf_store* table, void* stream);
/* ABI 13 -- the descriptor of a cropped keyframe store (described with its entry points at the end of this file) */
typedef struct objnerf_kf_crops {
  uint8_t* base; int64_t cap; int32_t* rect; float* t_wc; float* bbox;
} objnerf_kf_crops;

/* A4 alone (ABI 7): sceneObject.sample_3d_points(sampled_rgbs, sampled_depth, origins, dirs_w) (vmap.py:456-554) on
 * pixels the caller has already gathered: sampled_rgbs [n_frames][n_px][4] u8 (rgb + state, vmap.py:421),
 * sampled_depth [n_frames][n_px], origins [n_frames][3], dirs_w [n_frames][n_px][3] (utils.origin_dirs_W).  Of `a` the
 * scalars n_frames, n_px, n_cam2surf, n_bins, surface_eps, stop_eps, min_bound, obj_center, obj_index, seed, draw, the
 * draws u / g (both or neither: neither = the seeded form) and the outputs out_rgb, out_depth, out_valid, out_labels,
 * out_z, out_pts (or out_origins + out_dirs [n][3]) and max_depth_ws (1 + 6 n floats) are used; everything that
 * describes the keyframe store is ignored.  sampled_partfeat is passed through by the host (the reference returns its
 * argument, vmap.py:554). */
int objnerf_sample_points(const objnerf_sample_args* a, const uint8_t* sampled_rgbs, const float* sampled_depth,
                          const float* origins, const float* dirs_w, void* stream);

/* ------------------------------------------------------------------------------------------
 * f-3  Frame ingestion (train.py:196-256 + sceneObject.__init__ / append_keyframe, vmap.py:29-257): one new frame is
 * written into a keyframe slot of EVERY object that is visible in it, in one launch.  Per object the reference
 * builds a state map from the instance image (1 = this object, 2 = unknown (-1), 0 = other; train.py:201-203) and
 * copies rgb + state, depth, the camera pose and the 2-D box into the slot.
 *   rgb [W][H][3] u8, depth [W][H], inst [W][H] int32, t_wc [16]: the frame (device, images stored transposed)
 *   items: DEVICE array of K records: the object's four store tensors (layouts of objnerf_sample_rays), the slot
 *   to write, the instance id that means "this object" and its 2-D box.  Slot selection (keyframe / live frame /
 *   pruning, vmap.py:166-257) is host bookkeeping and stays with the caller.
 */
typedef struct objnerf_ingest_item {
  uint8_t* rgbs; float* depth; float* t_wc; float* bbox;
  int32_t slot, obj_id;
  float box[4];
} objnerf_ingest_item;
int objnerf_ingest_frame(int32_t W, int32_t H, const uint8_t* rgb, const float* depth, const int32_t* inst,
                         const float* t_wc, int32_t K, const objnerf_ingest_item* items, void* stream);

/* ------------------------------------------------------------------------------------------
 * f-1  Trainer.sample_points_bbox (trainer.py:130-198), the sampler of render_2D_syn (vmap.py:604-685).
 * objnerf_box_rays: P camera rays dirs_C [P][3] (un-normalised, rays_dir_cache[pixels]) of ONE view against an
 *   oriented box: T_WC, T_OC = inverse(T_WO) @ T_WC (both [4][4] row-major, computed by the caller as
 *   trainer.py:152-157 does), half = extent / 2.  Outputs: dirs_W [P][3] (origin_dirs_W, utils.py:324-336),
 *   near [P] (clipped at 0), far [P] (+0.2, :166-167), hit [P] u8 (ray_box_intersection, utils.py:309-319).
 * objnerf_box_points: for the n hit rays (compacted by the caller): z_vals [n][n_bins-1] = mid-points of
 *   stratified_bins(near, far, n_bins) with the injected draw u [n][n_bins] (utils.py:342-379, trainer.py:171-175;
 *   u == NULL: Philox draws of (seed; draw; ray, bin) generated in place) and pts [n][n_bins-1][3] = origin +
 *   dirs_W * z (:176).
 */
int objnerf_box_rays(int64_t P, const float* T_WC, const float* T_OC, const float* half_extent,
                     const float* dirs_C, float* out_dirs_W, float* out_near, float* out_far,
                     uint8_t* out_hit, void* stream);
int objnerf_box_points(int64_t n, int32_t n_bins, const float* origin /* [3] */, const float* dirs_W,
                       const float* near, const float* far, const float* u, uint64_t seed, uint32_t draw,
                       float* out_z, float* out_pts, void* stream);

/* f-1 in ONE launch (ABI 6): sceneObject.render_2D_syn's per-object chain (vmap.py:644-676) for the n hit rays of
 * objnerf_box_rays -- the 149 mid-points of Trainer.sample_points_bbox (trainer.py:171-176; u [n][n_bins] injected, or
 * NULL: the Philox draws of objnerf_box_points under (seed, draw)), UniDirsEmbed + OccupancyMap (embedding.py:46-55,
 * model.py:61-103), occupancy_activation / occupancy_to_termination / render (render_rays.py:6-63) -- with a lane per
 * ray and nothing per sample in HBM.  params: ONE object's block, scale [1].  Outputs per ray: depth, opacity, rgb [3]
 * and (out_hfeat != NULL) the composited hidden of the feature branch [n][H]: the 512-d map is objnerf_feature_head of
 * it with weight = opacity (exact: that head is linear).  out_z [n][n_bins-1] optional (the z_vals of the call).
 * Hidden 32 only (OBJNERF_ENOTSUP otherwise: wider networks keep objnerf_box_points -> objnerf_eval_points_ws ->
 * objnerf_composite).  mode: 0 = the reference's fp32 arithmetic (1e-4 parity, fixture G11); OBJNERF_TRAIN_BF16 = opt-in:
 * the operands of every hidden nn.Linear rounded to bf16 (v_mfma_f32_16x16x32_bf16, fp32 accumulation), sin / cos /
 * sigmoid on the transcendental unit -- the arithmetic of the bf16 training mode, fp32 compositing. */
int objnerf_render_fwd(const objnerf_net* net, int64_t n, int32_t n_bins, const float* params, const float* scale,
                       const float* origin /* [3] */, const float* dirs_W, const float* near, const float* far,
                       const float* u, uint64_t seed, uint32_t draw, float* out_depth, float* out_opacity,
                       float* out_rgb, float* out_hfeat, float* out_z, int32_t mode, void* stream);

/* ------------------------------------------------------------------------------------------
 * A6+A7  UniDirsEmbed.forward + OccupancyMap.forward (embedding.py:46-55, model.py:61-103),
 * inference: K objects x N points each.
 *   params [K][P_stride], scale [K] (pe buffer `scale`), pts [K][N][3]
 *   out_alpha [K][N] (= 10*raw, model.py:88), out_color [K][N][3] (sigmoid applied),
 *   out_hfeat [K][N][H] = relu(clip_linear(.)) or NULL, out_clip [K][N][C] = out_clip(.) or NULL.
 * This is what Trainer.eval_points (trainer.py:105-128) and render_2D_syn (vmap.py:644-655) run.
 */
int objnerf_eval_points(const objnerf_net* net, int32_t K, int64_t N, const float* params,
                        int64_t p_stride, const float* scale, const float* pts, float* out_alpha,
                        float* out_color, float* out_hfeat, float* out_clip, void* stream);

/* The same for ANY hidden width that is a multiple of 32 (the background network of trainer.py:15-17 is 128
 * wide and is rendered by the same render_2D_syn, vmap.py:644-655): hidden 32 runs the fused kernel above and
 * needs no workspace; wider networks run layer by layer with activations in the caller's workspace of
 * objnerf_eval_workspace_bytes(net, K, N) bytes (256-byte aligned). */
size_t objnerf_eval_workspace_bytes(const objnerf_net* net, int32_t K, int64_t N);
int objnerf_eval_points_ws(const objnerf_net* net, int32_t K, int64_t N, const float* params,
                           int64_t p_stride, const float* scale, const float* pts, float* out_alpha,
                           float* out_color, float* out_hfeat, float* out_clip, void* workspace,
                           size_t workspace_bytes, void* stream);

/* A7 alone: OccupancyMap.forward on a caller-supplied embedding emb [K][N][129] (model.py:61-103, the
 * call vmap(fc_model)(fc_param, fc_buffer, batch_embedding) of train.py:425).  Outputs as above. */
int objnerf_mlp_forward(const objnerf_net* net, int32_t K, int64_t N, const float* params,
                        int64_t p_stride, const float* emb, float* out_alpha, float* out_color,
                        float* out_hfeat, float* out_clip, void* stream);

/* The same for any hidden width that is a multiple of 32 (the reference calls scene_bg.trainer.fc_occ_map(bg_embedding)
 * on the 128-wide background network, train.py:449-450): hidden 32 runs the fused kernel and needs no workspace, wider
 * networks the layer-wise chain with objnerf_eval_workspace_bytes(net, K, N) bytes of caller workspace. */
int objnerf_mlp_forward_ws(const objnerf_net* net, int32_t K, int64_t N, const float* params,
                           int64_t p_stride, const float* emb, float* out_alpha, float* out_color,
                           float* out_hfeat, float* out_clip, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ABI 5 -- the BACKWARD halves of the two mirrored modules, for a caller that keeps the reference's loop body
 * (train.py:424-436: vmap(pe_model) -> vmap(fc_model) -> step_batch_loss -> loss.backward()) instead of the fused
 * objnerf_train_step: what autograd runs through model.py:61-103 and embedding.py:46-55.  fp32, any hidden width that
 * is a multiple of 32.
 *   emb      [K][N][129]  the embedding the forward entry was given (activations are recomputed from it),
 *   d_alpha  [K][N]       dL / d alpha   (alpha = the 10x-scaled occupancy logit objnerf_mlp_forward returns),
 *   d_color  [K][N][3]    dL / d color   (post-sigmoid),
 *   d_clip   [K][N][C]    dL / d out_clip, or NULL: the feature branch (tensors 14..17) then receives no gradient
 *                         and its slots of `grads` are left untouched,
 *   grads    [K][p_stride]  gradient arena in objnerf_param_layout order, tensors 0..13 (0..17 with d_clip) overwritten,
 *   d_emb    [K][N][129]  dL / d emb, overwritten (feed it to objnerf_embed_bwd).
 * workspace: objnerf_mlp_backward_workspace_bytes(net, K, N, d_clip != NULL) bytes, 256-byte aligned. */
size_t objnerf_mlp_backward_workspace_bytes(const objnerf_net* net, int32_t K, int64_t N, int32_t with_clip);
int objnerf_mlp_backward_ws(const objnerf_net* net, int32_t K, int64_t N, const float* params,
                            int64_t p_stride, const float* emb, const float* d_alpha, const float* d_color,
                            const float* d_clip, float* grads, float* d_emb, void* workspace,
                            size_t workspace_bytes, void* stream);

/* d B [K][21][3] of UniDirsEmbed.B_layer.weight (embedding.py:36-38) from d_emb [K][N][129] and the inputs of
 * objnerf_embed; scratch: K * 64 floats.  (d pts: objnerf_embed_bwd_pts, below.) */
int objnerf_embed_bwd(const objnerf_net* net, int32_t K, int64_t N, const float* params, int64_t p_stride,
                      const float* scale, const float* pts, const float* d_emb, float* d_B, float* scratch,
                      void* stream);

/* A6 alone: emb [K][N][3+21*n_freqs]. */
int objnerf_embed(const objnerf_net* net, int32_t K, int64_t N, const float* params,
                  int64_t p_stride, const float* scale, const float* pts, float* out_emb,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * A8+A9+A10  occupancy_activation -> occupancy_to_termination -> render (render_rays.py:6-63,
 * loss.py:27-35,82) for n_rays rays of S samples:
 *   alpha [n][S], color [n][S][3], z [n][S], vals [n][S][V] or NULL (any per-sample vector to
 *   composite: the H-wide feature hidden, or the reference's C-wide clip tensor).
 *   out_term [n][S] or NULL, out_depth/out_var/out_opacity [n], out_rgb [n][3], out_vals [n][V].
 */
#define OBJNERF_COMPOSITE_INPUT_IS_OCCUPANCY 1   /* `alpha` already holds sigmoid(alpha) (render_rays.py:32) */
int objnerf_composite(int64_t n_rays, int32_t S, int32_t flags, const float* alpha, const float* color,
                      const float* z, const float* vals, int32_t V, float* out_term,
                      float* out_depth, float* out_var, float* out_rgb, float* out_opacity,
                      float* out_vals, void* stream);

/* Measurement support (bench.py `roofline.peak_measured`; nothing in the reference): a saturated-MFMA loop, n_wg
 * workgroups of 4 waves x iters x 4 MFMAs on two accumulator chains per wave; dtype 0: v_mfma_f32_32x32x2_f32 (4096 FLOP
 * each), 1: v_mfma_f32_32x32x16_bf16 (32768 FLOP each) -- the instructions of the training kernels.  sink: n_wg * 256
 * floats. */
int objnerf_mfma_peak(int32_t dtype, int32_t iters, int32_t n_wg, float* sink, void* stream);

/* A8 alone: occupancy_activation(alpha) = sigmoid(alpha), n elements (render_rays.py:6-14). */
int objnerf_occupancy(int64_t n, const float* alpha, float* out, void* stream);

/* out_clip head applied after compositing (exact: the head is linear):
 * out [K][n][C] = of_w[k] . hfeat[k][n] + of_b[k] * weight[k][n]   (weight = opacity, or NULL=1). */
int objnerf_feature_head(const objnerf_net* net, int32_t K, int64_t n, const float* params,
                         int64_t p_stride, const float* hfeat, const float* weight, float* out,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * A11  loss.step_batch_loss (loss.py:5-103) on materialised network outputs:
 *   alpha [K][R][S], color [K][R][S][3], z [K][R][S], gt_depth [K][R], gt_rgb [K][R][3],
 *   labels [K][R] u8 (0 other / 1 this / 2 unknown), optional pred_feat [K][R][S][C] + gt_feat
 *   [K][R][C].  Scalings as loss.py:6.
 * Outputs: loss_terms [K][4] = per-object (depth, colour, opacity, feature) means, total [1],
 *   optional d_alpha / d_color / d_pred_feat (gradients of `total`), status [1] int32: bit 0 when a
 *   per-object term exceeds 1e5 (render_rays.py:109-111 "loss explode": the reference exits), bit 1 when a term is
 *   not finite (the reference's `> 100000` test is False for NaN and it carries on).  The same word, with the same
 *   two bits, is written by every entry point that has a `status` argument.
 * The cross-object early return (render_rays.py:89-94) is applied: if ANY object has no label-1
 * ray the depth / colour / feature terms are zero for ALL objects, likewise label!=2 for opacity.
 * counts: int32 workspace of 2*K + 2 entries; receives [K][2] = (n_label1, n_label_not2) and the two
 * early-return flags.
 * flags_in: optional [2] int32 "some object elsewhere (other GPU) had an empty mask".
 */
typedef struct objnerf_loss_args {
  int32_t K, R, S, C;
  float color_scaling, opacity_scaling, feat_scaling, reserved;
  const float* alpha; const float* color; const float* z; const float* gt_depth;
  const float* gt_rgb; const uint8_t* labels; const float* pred_feat; const float* gt_feat;
  const int32_t* flags_in;
  const int32_t* counts_in;   /* optional [K][2]: use these (e.g. all-reduced over GPUs that split one object's rays)
                                 instead of counting this call's labels */
  float* loss_terms; float* total; float* d_alpha; float* d_color; float* d_pred_feat;
  int32_t* counts; int32_t* status;
} objnerf_loss_args;
int objnerf_step_batch_loss(const objnerf_loss_args* a, void* stream);

/* Label statistics alone: counts [K][2], flags_out [2] (1 = some object has an empty mask). */
int objnerf_label_counts(int32_t K, int32_t R, const uint8_t* labels, int32_t* counts,
                         int32_t* flags_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * A12  one training iteration, fused: train.py:424-472 (vmap(pe) -> vmap(fc) -> step_batch_loss
 * -> backward) for K stacked objects in ONE pass over the rays.
 *
 * Inputs: params/scale as above; either pts [K][R][S][3] (train.py:397 batch_input_pcs) or, when
 * pts == NULL, origins [K][R][3] + dirs [K][R][3] + z (pts = o + d*z - center, vmap.py:548-551);
 * z [K][R][S]; gt_depth, gt_rgb, labels as objnerf_step_batch_loss; gt_feat [K][R][C] or NULL
 * (NULL = cfg.part_mode off: the feature branch gets no gradient, train.py:435-438).
 * counts [K][2] + flags [2]: from objnerf_label_counts (flags may have been max-reduced across
 * GPUs first -- the early return spans every object of the batch).
 * Outputs: grads [K][P_stride] (same layout as params; entries of tensors without gradient are
 * left untouched), loss_terms [K][4], status [1] (bits as objnerf_step_batch_loss: 0 = a term above 1e5, 1 = a term
 * that is not finite; every path of this entry point -- fused hidden 32, one-launch hidden 128, layer-wise, fused
 * hidden 256 -- writes both).  The fused fp32 hidden-32 kernel without the feature loss does not evaluate rays the loss
 * masks out (label 2: nothing of the ray; label 0: not its colour): with finite inputs that changes no bit of any
 * output; a value that is NOT finite and confined to a label-2 ray (NaN points, z, gt_depth or gt_rgb) need no
 * longer reach a loss term -- it does not where the ray's samples fill whole waves and its compositing pass holds only
 * label-2 rays, as at 64 samples per ray -- so bit 1 may stay clear for it there, while the other paths, which multiply
 * it by the zero mask, set it.
 * workspace: objnerf_train_workspace_bytes() bytes, 256-byte aligned (its with_feat argument: bit 0 = feature
 * loss, bit 1 = size for OBJNERF_TRAIN_LAYERWISE, bit 2 = size for the 16-bit modes only -- at hidden 256 they keep
 * the five activation and five gradient buffers in the operand type, a third less; a workspace sized without bit 2 serves every mode).
 */
#define OBJNERF_TRAIN_BF16 1   /* mode bit: MFMA operands rounded to bf16 (fp32 accumulate, fp32 master weights,
                                * fp32 embedding/compositing/losses).  NOT the reference's arithmetic (fp32,
                                * train.py:74) -- an opt-in throughput mode gated by PSNR.  Fused kernel: hidden 32,
                                * S <= 64, no feature loss (else OBJNERF_ENOTSUP); layer-wise path (other widths,
                                * longer rays): bf16 GEMM operands, any configuration. */
#define OBJNERF_TRAIN_FP16 4   /* mode bit: the layer-wise path with fp16 GEMM operands (v_mfma_f32_16x16x32_f16), fp32
                                * accumulate, fp32 master weights / activations / losses (BASELINE configs[4] names
                                * fp16).  Any width and ray length; implies the layer-wise path.  Operands saturate at
                                * +-65504 and the backward GEMMs scale their gradient operand by ~8 R (a power of two)
                                * so that it stays in fp16's normal range.  PSNR-gated like OBJNERF_TRAIN_BF16; not
                                * together with it (OBJNERF_EINVAL). */
#define OBJNERF_TRAIN_LAYERWISE 2   /* mode bit: take the layer-wise (any width) path even for hidden 32 / S <= 64 --
                                     * a second, independent implementation of the same iteration; the tests use
                                     * it to cross-check the fused kernel at sizes no CPU oracle reaches. */
#define OBJNERF_TRAIN_SELF_COUNTS 8   /* mode bit (ABI 7): the step derives the label statistics itself -- `counts` [K][2] and
                                       * `flags` [2] are then OUTPUTS (n(label == 1), n(label != 2) per object; the two
                                       * early-return flags of render_rays.py:89-94 over the K objects of THIS call), written
                                       * before anything of the step reads them: no objnerf_label_counts launch by the caller.
                                       * For an un-sharded batch only (under object sharding the flags span every rank's
                                       * objects and the background's counts every rank's rays: reduce them and pass them in). */
/* Helper streams + events for objnerf_train_step (see the preamble): create on the device that will run the steps,
 * destroy when no step using it is in flight.  The only entries of the library that create or free anything. */
struct objnerf_context;
int objnerf_context_create(struct objnerf_context** out);
int objnerf_context_destroy(struct objnerf_context* ctx);

/* ABI 7 -- the optimiser step of the iteration (train.py:472-473: optimiser.step() right after loss.backward()) inside
 * objnerf_train_step: the launch that reduces the partial gradients applies torch.optim.AdamW to the element it has
 * just summed (objnerf_adamw_step_flags' arithmetic, the same flag-dependent skipping and per-group step counters), so
 * an iteration has no separate optimiser launch and the gradient is not read back from HBM.  `grads` is still written.
 * group_steps / bank as in objnerf_adamw_step_flags (the caller alternates `bank`).  Tensors that receive no gradient
 * in the call's configuration (the feature branch without gt_feat) are skipped like a None .grad. */
typedef struct objnerf_adamw_args {
  float* exp_avg; float* exp_avg_sq;      /* [K][p_stride] like params */
  int32_t* group_steps; int32_t bank; int32_t reserved;
  float lr, beta1, beta2, eps, weight_decay, reserved_f;
} objnerf_adamw_args;

typedef struct objnerf_train_args {
  int32_t K, R, S, mode;
  float color_scaling, opacity_scaling, feat_scaling, obj_center;
  const float* params; int64_t p_stride; const float* scale;
  const float* pts; const float* origins; const float* dirs; const float* z;
  const float* gt_depth; const float* gt_rgb; const uint8_t* labels; const float* gt_feat;
  const int32_t* counts; const int32_t* flags;
  float* grads; float* loss_terms; int32_t* status;
  void* workspace; size_t workspace_bytes;
  uint8_t* relu_masks;   /* NULL in production.  Test hook, [K][R][S][6][hidden / 8] bytes: bit (f & 7) of byte
                          * f >> 3 of layer l (h1, h2, h3, h4, colour hidden, feature hidden -- the last only with
                          * gt_feat) is set iff that ReLU passed its input for the sample.  The parity tests evaluate
                          * the oracle on the SAME branches (an fp32 implementation and the reference legitimately
                          * disagree about inputs within rounding of zero; tests/parity_util.py).  Not with
                          * OBJNERF_TRAIN_BF16. */
  struct objnerf_context* context;   /* NULL: everything on `stream`.  Else the layer-wise path (hidden != 32,
                                      * S > 64, OBJNERF_TRAIN_LAYERWISE) forks its weight-gradient GEMMs and the feature
                                      * preparation onto the context's streams; one context serves one call at a time. */
  /* ABI 4 */
  float* emb_debug;      /* NULL in production.  Test hook, [K][R][S][129]: the fused fp32 kernel (hidden 32, S <= 64)
                          * writes the embedding rows its tiles computed IN REGISTERS (embedding.py:46-55 in the
                          * reference's column order) -- the kernel never materialises them otherwise, so this is the
                          * only way to compare its positional encoding with fixture G1.  Every other path refuses it
                          * (OBJNERF_ENOTSUP): their embedding is objnerf_embed's output. */
  /* ABI 7 */
  const objnerf_adamw_args* optim;   /* NULL: gradients only.  Else `params` (declared const for the gradient-only
                          * form) is UPDATED in place by the step's last launch, after every kernel that reads it. */
} objnerf_train_args;
size_t objnerf_train_workspace_bytes(const objnerf_net* net, int32_t K, int32_t R, int32_t S,
                                     int32_t with_feat);
int objnerf_train_step(const objnerf_net* net, const objnerf_train_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * A12  torch.optim.AdamW.step as train.py:78 configures it (lr, weight_decay; betas .9/.999,
 * eps 1e-8), over the arena.  has_grad [P] u8: 0 for tensors that received no gradient this
 * iteration (they get NO update and NO decay, like a None .grad).  step = 1-based step count.
 */
int objnerf_adamw_step(int32_t K, int64_t P, int64_t p_stride, float* params, const float* grads,
                       float* exp_avg, float* exp_avg_sq, const uint8_t* has_grad, int32_t step,
                       float lr, float beta1, float beta2, float eps, float weight_decay,
                       void* stream);

/* The same step with the early-return quirk of render_rays.py:89-94 carried through to the optimiser: `flags` is the
 * iteration's device flag pair (objnerf_label_counts / the all-reduced flags).  flags[0] set = the depth, colour and
 * feature terms were constants this iteration: the colour branch [colour_lo, feature_lo) and the feature branch
 * [feature_lo, feature_hi) of every object had .grad = None in the reference, and torch.optim.AdamW skips such
 * parameters entirely (no decay, no moment update, no step increment); both flags set = nothing is updated.
 * group_steps: device int32[2][3]: two banks of per-group step counters (trunk + density head + B | colour | feature),
 * zero-initialised by the caller.  The call reads bank `bank` (0 / 1) and writes the advanced counters to the other
 * one: the caller alternates `bank` from call to call, starting with 0 (one launch, no counter is read after it moved).
 * has_grad still masks what a configuration never differentiates. */
int objnerf_adamw_step_flags(int32_t K, int64_t P, int64_t p_stride, float* params, const float* grads, float* exp_avg,
                             float* exp_avg_sq, const uint8_t* has_grad, const int32_t* flags, int32_t* group_steps,
                             int32_t bank, int64_t colour_lo, int64_t feature_lo, int64_t feature_hi, float lr,
                             float beta1, float beta2, float eps, float weight_decay, void* stream);

/* ------------------------------------------------------------------------------------------
 * Helper functions of the reference's call surface that a caller may use outside the fused iteration
 * (objnerf_helpers.hip).  All take / return device pointers; small HBM-bound kernels.
 */
/* render_rays.render (render_rays.py:56-63): out [n_rays][C] = sum over the S samples of termination [n_rays][S] *
 * vals [n_rays][S][C] (C = 1 for depth-like quantities). */
int objnerf_render(int64_t n_rays, int32_t S, int32_t C, const float* termination, const float* vals, float* out,
                   void* stream);

/* render_rays.render_loss (render_rays.py:65-83).  mode 0 "L1": |render - gt|, 1 "L2": squared, n elements;
 * mode 2 "cos": 1 - cosine_similarity over rows of C entries (norms clamped at 1e-8), n rows.  normalise: / gt. */
int objnerf_render_loss(int64_t n, int32_t C, int32_t mode, int32_t normalise, const float* render, const float* gt,
                        float* out, void* stream);
/* render_rays.reduce_batch_loss (render_rays.py:85-117): loss_mat [K][R], var [K][R] or NULL (information weight
 * 1 / (sqrt(var) + 1e-4), or 1 / (var + 1e-4) with l2), mask [K][R] u8.  avg: out [K] = masked means, all zero when
 * ANY object's mask is empty (:89-94); status bit 0 set when a mean exceeds 1e5 (:109-111, the reference exits), bit 1
 * when a mean is not finite.
 * avg == 0: out [K][R] = the weighted matrix.  counts_ws: K + 1 ints of scratch. */
int objnerf_reduce_batch_loss(int32_t K, int32_t R, const float* loss_mat, const float* var, const uint8_t* mask,
                              int32_t l2, int32_t avg, int32_t* counts_ws, float* out, int32_t* status, void* stream);
/* render_rays.make_3D_grid (render_rays.py:119-146): out [dim][dim][dim][3] = lattice on [lo, hi]^3, optionally
 * scaled per axis (scale [3]) and moved by transform [4][4] (row-major). */
int objnerf_make_grid(int32_t dim, float lo, float hi, const float* scale, const float* transform, float* out,
                      void* stream);
/* utils.ray_box_intersection (utils.py:309-319): n rays against the axis-aligned box [bmin, bmax] ([3] each). */
int objnerf_ray_box(int64_t n, const float* origins, const float* dirs, const float* bmin, const float* bmax,
                    float* out_near, float* out_far, uint8_t* out_hit, void* stream);
/* utils.origin_dirs_W (utils.py:324-336): out_dirs_W [F][P][3] = R_wc[f] dirs_C[f][p]  (T_WC [F][4][4]; the
 * origins are T_WC[:, :3, 3], a view on the caller's side). */
int objnerf_dirs_w(int64_t F, int64_t P, const float* T_WC, const float* dirs_C, float* out_dirs_W, void* stream);
/* utils.stratified_bins (utils.py:342-379): out [n_rays][n_bins] = lo + range * i / n + U * range / n; lo / hi per
 * ray or NULL (then the scalar); U = u [n_rays][n_bins] (injected draws) or, with u == NULL, the counter-based
 * generator of objnerf_philox.h under (seed, offset). */
int objnerf_stratified_bins(int64_t n_rays, int32_t n_bins, const float* lo, float lo_scalar, const float* hi,
                            float hi_scalar, const float* u, uint64_t seed, uint64_t offset, float* out, void* stream);
/* utils.normal_bins_sampling (utils.py:382-397): out [n_rays][n_bins] = depth + clip(sort(N(0, (delta/3)^2)), +-delta);
 * g = injected draws (already scaled) or NULL for the counter-based generator. */
int objnerf_normal_bins(int64_t n_rays, int32_t n_bins, const float* depth, float delta, const float* g, uint64_t seed,
                        uint64_t offset, float* out, void* stream);

/* ABI 8 -- marching cubes (vis.py:6-22: skimage.measure.marching_cubes(occupancy, level, gradient_direction='ascent'),
 * as Trainer.meshing calls it, trainer.py:46-103) on a device fp32 volume vol [dim][dim][dim], last axis fastest
 * (occ.view(grid_dim, grid_dim, grid_dim), trainer.py:81), 2 <= dim <= 1024.  Output in index units, welded: one
 * vertex per lattice edge whose endpoints straddle the level (a corner is above when its value > level), ordered by
 * (owning lattice point, axis); faces ordered by (cell, table order); bit-reproducible, no atomics.
 * objnerf_mc_workspace_bytes: the workspace both calls share (0 for a dim outside the range).
 * objnerf_mc_count: out_counts (device int64 [2]) = V, F; leaves per-workgroup offsets in ws.
 * objnerf_mc_emit: only valid after objnerf_mc_count with the same dim, level, vol and ws.  out_verts [V][3] fp32,
 * out_normals [V][3] fp32 (unit, down the gradient, as skimage's), out_faces [F][3] int32; nothing is written past
 * max_verts / max_faces rows.  The caller keeps V <= 2^31 - 1 (int32 face indices).  flags: OBJNERF_MC_DESCENT
 * writes every face reversed (gradient_direction='descent'). */
#define OBJNERF_MC_DESCENT 1
size_t objnerf_mc_workspace_bytes(int32_t dim);
int objnerf_mc_count(int32_t dim, float level, const float* vol, void* ws, size_t ws_bytes, int64_t* out_counts,
                     void* stream);
int objnerf_mc_emit(int32_t dim, float level, int32_t flags, const float* vol, void* ws, size_t ws_bytes,
                    int64_t max_verts, int64_t max_faces, float* out_verts, float* out_normals, int32_t* out_faces,
                    void* stream);
/* host only: copies of the compiled case table (objnerf_mc_tables.h; any pointer may be NULL): edge_c0 [12],
 * edge_axis [12], ntri [256], tri [256][3 * max_tris] (0xff past a case's triangles).  Returns max_tris. */
int objnerf_mc_tables(uint8_t* edge_c0, uint8_t* edge_axis, uint8_t* ntri, uint8_t* tri);

/* ABI 9 -- object bounds from keyframes (objnerf_bounds.hip): sceneObject.get_bound (vmap.py:287-384), which the
 * reference runs on the CPU per object through open3d (create_from_depth_image + voxel_down_sample, :303-320) and
 * trimesh.bounds.oriented_bounds (:330-334).
 *
 * (a) Voxel centroids of K objects' keyframe point clouds (vmap.py:303-320).  `table` [K] (device): the objects'
 * keyframe stores (objnerf_kf_store; rgbs and depth are read, F slots of [W][H] each); n_keyframes [K] (device): only
 * slots 0 .. n_keyframes-1 are read; camera_pose [K][F][16] (device, row-major) = inv64(inv32(twc)) per slot, as open3d
 * receives it (vmap.py:307-310).  A pixel (row i, column j) belongs to the cloud when its state byte is 1 and its depth
 * z > 0 (NaN fails); point = camera_pose (x, y, z, 1), x = (j - cx) z / fx, y = (i - cy) z / fy, all in fp64 without
 * contraction; points in the order (slot, i, j).
 * objnerf_voxel_workspace_bytes: the workspace scan and emit share.
 * objnerf_voxel_scan: out_total [K] (device int64) = point counts, out_minmax [K][6] (device fp64) = min xyz, max xyz
 * (+inf / -inf for an empty cloud).
 * objnerf_voxel_emit: the points of objects k0 .. k1-1 (after a scan with the same arguments): object k's points go to
 * rows base[k] .. base[k] + total[k] - 1 of out_pts [n_points][3] (fp64), in the cloud's order, with out_keys [n_points]
 * = (k - k0) << 42 | (ix + dims[k][0] (iy + dims[k][1] iz)), ixyz = floor((p - vmin[k]) / voxel) (open3d's voxel
 * index; vmin [K][3], dims [K][2] device).  Nothing is written past n_points rows.
 * objnerf_voxel_heads: for keys sorted ascending with equal keys in cloud order (a stable sort of out_keys): ws
 * (objnerf_voxel_heads_workspace_bytes(n)) receives per-block offsets of the distinct keys, ws[last] = their count V.
 * objnerf_voxel_centroids: one row per distinct key, in key order (V <= max_voxels rows written): out_centroids
 * [V][3] = the in-order fp64 sum of the key's points (perm = the sort's permutation into out_pts) / their count
 * (voxel_down_sample, vmap.py:320), out_keys [V] = the key's low 42 bits, out_first[k - k0] = the first row of object k
 * (left untouched for an object without points). */
typedef struct objnerf_voxel_args {
  int32_t K, F, W, H;
  double fx, fy, cx, cy, voxel;
  const objnerf_kf_store* table; const int32_t* n_keyframes; const double* camera_pose;
  /* ABI 13 -- crops [K] (device) in place of table (which may then be NULL): the objects' cropped keyframe stores.  Scan
   * and emit read only the pixels inside each slot's rect, a tile that does not meet the rect is not loaded at all; the
   * points, their order and every output are those of the dense store with the same pixels. */
  const objnerf_kf_crops* crops;
} objnerf_voxel_args;
size_t objnerf_voxel_workspace_bytes(int32_t K, int32_t F, int32_t W, int32_t H);
int objnerf_voxel_scan(const objnerf_voxel_args* a, void* ws, size_t ws_bytes, int64_t* out_total, double* out_minmax,
                       void* stream);
int objnerf_voxel_emit(const objnerf_voxel_args* a, const void* ws, size_t ws_bytes, int32_t k0, int32_t k1,
                       const int64_t* base, const double* vmin, const int64_t* dims, int64_t n_points, double* out_pts,
                       int64_t* out_keys, void* stream);
size_t objnerf_voxel_heads_workspace_bytes(int64_t n);
int objnerf_voxel_heads(int64_t n, const int64_t* sorted_keys, int64_t* ws, void* stream);
int objnerf_voxel_centroids(int64_t n, const int64_t* sorted_keys, const int64_t* perm, const double* pts,
                            const int64_t* ws, int64_t max_voxels, double* out_centroids, int64_t* out_keys,
                            int64_t* out_first, void* stream);

/* (b) Oriented-box search for K point sets (trimesh.bounds.oriented_bounds(points, ordered=True), vmap.py:330-334,
 * over an exact candidate set): verts [V][3] fp64 hull vertices, object k's rows vert_off[k] .. vert_off[k+1]-1;
 * normals [N][3] unit (global rows); edges [E][2] int32 vertex indices local to the object; cand [C][2] int32 =
 * (global normal row, global edge row), object k's rows cand_off[k] .. cand_off[k+1]-1; mode [K]: 0 = minimise the
 * volume, 1 = a coplanar set (one normal, height 0): minimise the (u, v) area.  Per candidate: u = e projected onto
 * the plane normal to n, normalised (skipped when degenerate), v = n x u; extents = max - min of the vertices'
 * projections on (u, v, n).  The minimum is taken in (criterion, candidate row) order.  ws: 2 K n_split doubles.
 * out [K][16] fp64: R [3][3] row-major with columns u, v, n; extents [3]; centre [3] (world); criterion (+inf: no
 * valid candidate).  All device pointers. */
typedef struct objnerf_obb_args {
  int32_t K, reserved;
  const double* verts; const int64_t* vert_off; const double* normals; const int32_t* edges; const int32_t* cand;
  const int64_t* cand_off; const int32_t* mode;
} objnerf_obb_args;
int objnerf_obb_search(const objnerf_obb_args* a, int32_t n_split, double* ws, double* out, void* stream);

/* ABI 10 -- open-vocabulary queries over the exported map (objnerf_query.hip): the numerical core of
 * visualization/vis_interaction.py, which the reference runs per object on the host (F.cosine_similarity :372-373,
 * :388; sim_and_update's min-max + matplotlib "rainbow" :329-332, :389-392; StandardScaler + PCA(3) + joint min-max
 * :205-216).  Segments are row ranges: segment s is rows seg_off[s] .. seg_off[s+1]-1 (device int64 [S+1], clamped to
 * [0, V]); an empty segment is allowed.  All pointers are device pointers unless stated; no float atomics, and two
 * calls with the same inputs write the same bytes.
 *
 * objnerf_project: out [V][Q] fp32 = f . W + bias for every row f of every segment; feat [V][D] fp32 with a row
 * stride (floats, >= D), 1 <= D <= 1024, 1 <= Q <= 16; W [D][Q] row-major, shared, or [S][D][Q] with
 * OBJNERF_PROJ_PER_SEGMENT (bias [Q] or [S][Q] likewise; NULL: none).  OBJNERF_PROJ_COSINE: f and every column of W
 * are divided by max(|.|, 1e-8) first (torch.nn.functional.cosine_similarity).  minmax [S][Q][2] = min, max of the
 * segment's rows of out (+inf / -inf for an empty segment).  Products on v_mfma_f32_16x16x4_f32 (fp32).  Rows outside
 * every segment are not written.  ws: objnerf_project_workspace_bytes(S, Q, V). */
#define OBJNERF_PROJ_COSINE 1
#define OBJNERF_PROJ_PER_SEGMENT 2
typedef struct objnerf_project_args {
  int32_t S, D, Q, flags;
  int64_t V, row_stride;
  const float* feat; const int64_t* seg_off; const float* W; const float* bias;
  float* out; float* minmax;
} objnerf_project_args;
size_t objnerf_project_workspace_bytes(int32_t S, int32_t Q, int64_t V);
int objnerf_project(const objnerf_project_args* a, void* ws, size_t ws_bytes, void* stream);

/* objnerf_moments: per segment, mean [S][D] fp64 (fp64 sums of contiguous row chunks, combined in chunk order) and
 * the centred scatter matrix scatter [S][D][D] fp64 = sum over the rows of (f - m)(f - m)^T, m = the mean rounded to
 * fp32: centred before the products (part features are unit vectors with a large common mean: X^T X - n m m^T in fp32
 * loses the spread); products and runs of 128 rows in fp32 on v_mfma_f32_16x16x4_f32, folded into fp64 in row order;
 * exactly symmetric.  An empty segment gives zeros.  ws: objnerf_moments_workspace_bytes(S, D). */
typedef struct objnerf_moments_args {
  int32_t S, D;
  int64_t V, row_stride;
  const float* feat; const int64_t* seg_off;
  double* mean; double* scatter;
} objnerf_moments_args;
size_t objnerf_moments_workspace_bytes(int32_t S, int32_t D);
int objnerf_moments(const objnerf_moments_args* a, void* ws, size_t ws_bytes, void* stream);

/* objnerf_vertex_colors: out [V][3] fp32 for the rows of every segment, by mode[s]:
 *   OBJNERF_COLOR_RGB      fp32(rgb[row][c] / 255 * factor[s]) in fp64 (rgb: uint8, rgb_stride bytes per row; the
 *                          reference's color[..., :3] / 255 * 0.8 (color_by_rgb) or * 0.5 (a non-selected object));
 *   OBJNERF_COLOR_CONSTANT constant[s][0..2];
 *   OBJNERF_COLOR_RAINBOW  matplotlib's "rainbow" of x = fp32(fp32(v - mn) / fp32(mx - mn)), v = proj[row][column[s]],
 *                          (mn, mx) = minmax[s][column[s]]: entry trunc(256 x) (256 -> 255), x < 0 -> 0, x > 1 -> 255,
 *                          NaN (a constant segment) -> (0, 0, 0); proj [V][Q];
 *   OBJNERF_COLOR_PCA      columns 0..2 of proj (Q >= 3), each negated when -min > max (the largest |score| positive),
 *                          normalised by one joint min / max over the three, clipped to [0, 1] (NaN -> 0).
 * Arrays a mode does not read may be NULL. */
#define OBJNERF_COLOR_RGB 0
#define OBJNERF_COLOR_CONSTANT 1
#define OBJNERF_COLOR_RAINBOW 2
#define OBJNERF_COLOR_PCA 3
typedef struct objnerf_color_args {
  int32_t S, Q;
  int64_t V, rgb_stride;
  const int64_t* seg_off; const int32_t* mode;
  const uint8_t* rgb; const double* factor; const float* constant; const int32_t* column;
  const float* proj; const float* minmax;
  float* out;
} objnerf_color_args;
int objnerf_vertex_colors(const objnerf_color_args* a, void* stream);
/* host only: the "rainbow" table the colour kernel uses, out [256][3] fp32 (matplotlib's _lut[:256, :3] rounded to
 * fp32).  Returns 256. */
int objnerf_rainbow_lut(float* out);

/* ABI 11 -- cross-frame mask association (objnerf_maskgraph.hip): the data-parallel parts of
 * maskclustering/mask_graph.py.  All pointers are device pointers; point sets are fp64 [n][3] rows grouped into
 * segments, segment s = rows seg_off[s] .. seg_off[s+1]-1 (device int64 [S+1], seg_off[0] = 0, seg_off[S] = n, an empty
 * segment is allowed), n < 2^31.  No float atomics; integer atomics only where the result does not depend on their
 * order; fp64 point arithmetic without contraction; two calls with the same inputs write the same bytes.
 *
 * objnerf_cell_keys: out_min [S][3] = the minimum corner of every segment (+inf for an empty one), out_keys [n] =
 * ix << 42 | iy << 21 | iz with i = floor((p - (min - shift)) / cell) per axis (shift >= 0: 0 for the two searches
 * below; voxel / 2 with cell = voxel gives open3d's voxel_down_sample indices, mask_graph.py:410, :1178).  status (one int32) is set to 1 when a point
 * is not finite or lies more than 2^21 - 1 cells from the corner (its key is then meaningless), else 0.  The caller
 * sorts the keys per segment (stable; rows stay inside their segment) and passes sorted keys and permutation
 * (perm[t] = the row at sorted position t) to the two entries below.  cell must be >= the search radius; pass the radius
 * times (1 + 2^-20) so that the rounding of the division cannot put two points within the radius two cells apart.
 *
 * objnerf_dbscan: pcd.cluster_dbscan(eps, min_points) (pcd_denoise_dbscan, mask_graph.py:244-316) for S point sets at
 * once.  A point is core when at least min_points[s] points of its segment, itself included, have d^2 <= eps^2;
 * clusters are the connected components of the core points, numbered per segment from 0 by their smallest core row,
 * ascending; a border point takes the lowest cluster id among its core neighbours; a point without core neighbour gets
 * -1: the labels of a sequential DBSCAN that visits the points in row order (scikit-learn's DBSCAN on the same
 * input).  labels int32 [n].  A segment with min_points[s] <= 0 is skipped and its labels are left as they are (the
 * fallback chain 100 -> 20 -> 10 re-runs only the segments that found no cluster, on the same sorted keys).
 * ws: objnerf_dbscan_workspace_bytes(n).
 *
 * objnerf_cloud_overlap: compute_similarity_matrix_thre's compute_point_cloud_distance(...) < dis_thre counts
 * (mask_graph.py:835-846) for all ordered pairs of C clouds (C <= 65535) in one launch: out_count [C][C] int64,
 * out_count[a][b] = the points of cloud a that have some point of cloud b at distance < dis_thre (strict; by
 * d^2 < dis_thre^2).  The keys come from objnerf_cell_keys with ONE segment over all rows (one grid for every cloud),
 * sorted per cloud. */
int objnerf_cell_keys(int64_t n, int32_t S, const double* pts, const int64_t* seg_off, double cell, double shift,
                      double* out_min, int64_t* out_keys, int32_t* status, void* stream);
size_t objnerf_dbscan_workspace_bytes(int64_t n);
int objnerf_dbscan(int64_t n, int32_t S, const double* pts, const int64_t* seg_off, const int64_t* sorted_keys,
                   const int64_t* perm, const int32_t* min_points, double eps, void* ws, size_t ws_bytes, int32_t* labels,
                   void* stream);
int objnerf_cloud_overlap(int64_t n, int32_t C, const double* pts, const int64_t* cloud_off, const int64_t* sorted_keys,
                          const int64_t* perm, double dis_thre, int64_t* out_count, void* stream);

/* objnerf_mask_ray_boxes: the ray / box pass of compute_2d_iou_matrix (mask_graph.py:683-710 with get_rays :562-571,
 * ray_box_intersection :634-643 and min_rect_bbox :660-680) for F frames and N mask boxes in one launch.  For frame f
 * a ray per 10th pixel: d = ((ix - cx) / fx, (iy - cy) / fy, 1) in fp32, widened to fp64 and multiplied by
 * depth[f][iy][ix] / 1000.0 (depth: the raw uint16 image [F][H][W]; 1000 is the reference's literal), rotated by
 * twc[f][:3,:3] (twc [F][4][4] fp64 row-major), origin twc[f][:3,3].  Slab test in fp64, IEEE semantics followed
 * literally (a zero depth gives infinities and NaNs; a NaN makes the comparisons false): t = (bound - origin) / d,
 * near = max over axes of min(tmin, tmax), far = min of max, hit = near <= far && far > 0.  boxes [N][6] fp64 (min, max).
 * out [F][N][4] int32 = (row_min, col_min, row_max + 1, col_max + 1) of the hit rays in the H/10 x W/10 ray grid, zeros
 * when no ray hits.  W or H not a multiple of 10: OBJNERF_EINVAL (the reference's view() fails on them).  F <= 65535. */
typedef struct objnerf_ray_boxes_args {
  int32_t F, N, W, H;
  double fx, fy, cx, cy;
  const uint16_t* depth; const double* twc; const double* boxes;
  int32_t* out;
} objnerf_ray_boxes_args;
int objnerf_mask_ray_boxes(const objnerf_ray_boxes_args* a, void* stream);

/* Mask clouds of one frame (project_mask_pc, mask_graph.py:337-462).  objnerf_mask_points: pix [n] int32 = v * W + u
 * of the pixels (the caller lists them in raster order per (mask, connected component) segment), depth [H][W] fp32
 * (already depth / depth_scale with values outside [0.07, 10] set to 0, :342-350), pose fp64 [4][4] row-major:
 * x = (u - cx) * d / fx, y = (v - cy) * d / fy, z = d in fp32, left to right without contraction (:375-377), then
 * out [n][3] fp64 = pose * (x, y, z, 1) (pcd.transform, :382), every product and sum rounded on its own.
 * objnerf_mask_hist: out [M][96] fp32 = per mask the 3 x 32 histogram (bins of width 8; channel order of img [H][W][3]
 * uint8, the reference's B, G, R) over the pixels pix[mask_off[m] .. mask_off[m+1]) -- the caller passes mask & depth > 0,
 * the mask before filtering (:451) -- integer counts written as fp32 (cv2.calcHist).
 * objnerf_point_bounds: out [S][6] fp64 = (min, max) of every segment's points (:441-442; +inf / -inf when empty). */
typedef struct objnerf_mask_points_args {
  int64_t n;
  int32_t W, H;
  double fx, fy, cx, cy;
  const int32_t* pix; const float* depth; const double* pose;
  double* out;
} objnerf_mask_points_args;
int objnerf_mask_points(const objnerf_mask_points_args* a, void* stream);
int objnerf_mask_hist(int64_t n, int32_t M, const int32_t* pix, const int64_t* mask_off, const uint8_t* img, int32_t W,
                      int32_t H, float* out, void* stream);
int objnerf_point_bounds(int64_t n, int32_t S, const double* pts, const int64_t* seg_off, double* out, void* stream);

/* objnerf_mask_affinity: the five N x N affinity matrices of mask_graph.py:1047-1054 and MaskGraph.__init__'s weighted
 * sum (:46) in one pass, W [N][N] fp32:
 *   geo    compute_3d_iou_matrix (:501-530): box intersection volume / the smaller volume in fp64, NaN -> 0;
 *          boxes [N][6] fp64;
 *   cap, clip  adjacent_matrix_feat (:573-584): x_i . x_j / (|x_i| |x_j|) in fp32, products on v_mfma_f32_16x16x4_f32,
 *          no epsilon (a zero row gives NaN, which makes no edge); cap [N][d_cap], clip [N][d_clip], widths 1 .. 1024;
 *   color  compute_color_matrix (:592-601): rows divided by their norm first, then the products; color [N][96];
 *   geo2d  compute_2d_iou_matrix's running mean m = (m * f + iou_f) / (f + 1) in fp32 in frame order (:712), iou_f =
 *          compute_iou_2d (:533-558) of boxes2d [F][N][4] int32 (objnerf_mask_ray_boxes): int32 areas, a true
 *          division in fp32, NaN -> 0; bit-equal to the recurrence.  Skipped (boxes2d may be NULL) when w_geo2d == 0.
 *   W = fp32(geo * w_geo + fp64(cap *f32 w_cap) + fp64(clip *f32 w_clip) + fp64(color *f32 w_color)
 *            + fp64(geo2d *f32 w_geo2d)): numpy's fp64 matrix plus float32 matrices times Python floats.
 * terms (NULL: not written) [5][N][N] fp32 = geo, cap, clip, color, geo2d.  Norms are fp32(sqrt(fp64 sum of squares)).
 * row_off [N+1] int64 = exclusive offsets of the rows' edge counts, edges being the pairs i < j with W[i][j] >= 1.0
 * (get_edges, :57-80; tested on the fp32 W); row_off[N] = their number.  objnerf_mask_edges then writes them in
 * row-major order: out_ij [E][2] int32, out_w [E] fp32 (entries past max_edges are dropped).
 * ws: objnerf_affinity_workspace_bytes(N).  No atomics; two calls write the same bytes. */
typedef struct objnerf_affinity_args {
  int32_t N, F, d_cap, d_clip;
  double w_geo, w_cap, w_clip, w_color, w_geo2d;
  const double* boxes; const float* cap; const float* clip; const float* color; const int32_t* boxes2d;
  float* W; float* terms;
} objnerf_affinity_args;
size_t objnerf_affinity_workspace_bytes(int32_t N);
int objnerf_mask_affinity(const objnerf_affinity_args* a, void* ws, size_t ws_bytes, int64_t* row_off, void* stream);
int objnerf_mask_edges(int32_t N, const float* W, const int64_t* row_off, int64_t max_edges, int32_t* out_ij, float* out_w,
                       void* stream);

/* ABI 12 -- compact part-level feature maps (objnerf_partmap.hip; partlevel/sam_clip_dir.py:113-133 of the reference).
 * objnerf_part_index: masks [M][Hp][Wp] uint8 (non-zero = set; already taken on the stride, mask[::d, ::d]) ->
 * out [Hp][Wp] int32 = the number of the LAST mask that covers the pixel (the reference assigns mask after mask, a later
 * one overwrites an earlier one), -1 where none does.  M = 0 is allowed (masks may then be NULL): all -1.
 * objnerf_part_dense: out [n_px][C] = table[index[p]], table [rows][C] fp32, index [n_px] int32 clamped to [0, rows):
 * with row 0 of the table zero and the index image shifted by one (0 = none) this is the reference's dense map.  A wave
 * per pixel, 16-byte lanes when C % 4 == 0 and table / out are 16-byte aligned.  No atomics in either. */
int objnerf_part_index(int32_t M, int32_t Hp, int32_t Wp, const uint8_t* masks, int32_t* out, void* stream);
int objnerf_part_dense(int64_t n_px, int32_t C, int32_t rows, const int32_t* index, const float* table, float* out,
                       void* stream);

/* ABI 13 -- cropped keyframe stores (openobj_amd/kf_store.py): an object keeps, per keyframe slot, only the pixels of
 * the slot's rect = the pixels the sampler can draw inside the slot's 2-D box (columns trunc(box[0]) .. trunc(box[1]),
 * rows trunc(box[2]) .. trunc(box[3]), clipped to the image).  base: the object's byte arena of F slots of cap * 8
 * bytes; slot s holds cap * 4 bytes of rgb + state followed by cap floats of depth, the crop row-major [cw][ch] (the
 * transposed orientation of the dense store): pixel (iw, ih) of the image is element (iw - x0) * ch + (ih - y0).
 * rect [F][4] int32 = {x0, y0, cw, ch} (cw * ch <= cap), t_wc [F][4][4] and bbox [F][4] as in objnerf_kf_store.
 *
 * objnerf_ingest_frame_crops: objnerf_ingest_frame for cropped stores, one launch for the K visible objects.  The
 * state byte of every (pixel, object) is computed as there; only the pixels inside items[k].rect are written, with
 * rect, pose and box of the slot.  A pixel OUTSIDE the rect whose state is 1 adds 1 to outside[k] (device int32 [K],
 * never cleared here: the caller keeps it across frames) -- such a pixel is lost to get_bound, the caller's box was
 * narrower than the instance.  The caller guarantees rect inside the image and rect[2] * rect[3] <= store.cap
 * (EINVAL is returned for what can be checked on the host: null pointers, sizes, K).
 *
 * objnerf_sample_rays_crops: objnerf_sample_rays_stacked reading cropped stores: same arguments, same draws, same
 * outputs stacked [K][...] (K = 1: the layouts of objnerf_sample_rays).  A pixel index outside the slot's rect (only
 * possible when the caller changed the box after ingest) is clamped into it; ray directions and the part-feature
 * gather use the image coordinates. */
typedef struct objnerf_ingest_crop_item {
  objnerf_kf_crops store;
  int32_t slot, obj_id;
  float box[4];
  int32_t rect[4];
} objnerf_ingest_crop_item;
int objnerf_ingest_frame_crops(int32_t W, int32_t H, const uint8_t* rgb, const float* depth, const int32_t* inst,
                               const float* t_wc, int32_t K, const objnerf_ingest_crop_item* items, int32_t* outside,
                               void* stream);
int objnerf_sample_rays_crops(const objnerf_sample_args* a, int32_t K, const objnerf_kf_crops* table, void* stream);

/* ABI 14 -- labelling arbitrary points against the whole map (objnerf_mappoints.hip; openobj_amd/map_points.py): for N
 * world points and K objects in the caller's order, the arg-max over objects of Trainer.eval_points (trainer.py:105-128)
 * restricted to each object's box -- the 3-D counterpart of the z-buffer merge of train.py:550-612.
 * boxes [K][16] fp32: center [3] | R [3][3] row-major | extent / 2 [3] | obj_center (the "bbox" of obj_<id>.pth,
 * vmap.py:556-576; obj_center as map_vis.export passes it to Trainer.meshing, trainer.py:60).
 *
 * objnerf_mappoints_count / _emit (two calls, as objnerf_mc_count / _emit): point n is a candidate of object k iff
 * |R_k^T (p_n - c_k)| <= extent_k / 2 in every component, in fp32.  count writes seg_off [K + 1] (device int64, exclusive,
 * seg_off [K] = M) and leaves per-workgroup offsets in ws; the caller reads M and allocates; emit (same N, K, pts, boxes
 * and ws) writes pair_pt [M] int32: object-major, ascending in the point index inside an object.  No atomics.
 * N <= 2^31 - 1, K <= 65535; EINVAL for M > 2^31 - 1 (the keys below hold a pair in 31 bits). */
size_t objnerf_mappoints_workspace_bytes(int64_t N, int32_t K);
int objnerf_mappoints_count(int64_t N, int32_t K, const float* pts, const float* boxes, void* ws, size_t ws_bytes,
                            int64_t* seg_off, void* stream);
int objnerf_mappoints_emit(int64_t N, int32_t K, const float* pts, const float* boxes, const void* ws, size_t ws_bytes,
                           int64_t M, int32_t* pair_pt, void* stream);
/* OccupancyMap.forward on UniDirsEmbed.forward (model.py:61-103, embedding.py:46-55) for every pair of the hidden-32
 * objects, at p - obj_center: a flat list of (object, 64-pair tile), weights staged per object, points gathered through
 * pair_pt.  info [K][2] int32: {row of the object in the arena `params` [rows][p_stride] / `scale` [rows], or -1 for an
 * object this call leaves out (a wider network); 1 for a background object (bg_ids of render_view), else 0}.
 * pair_alpha [M] = 10 * raw (model.py:88); pair_color [M][3] (sigmoid applied) and pair_hfeat [M][32] (the input of
 * out_clip, model.py:100) may be NULL.  best [N] uint64, ZEROED BY THE CALLER before the first eval / merge of a cloud,
 * receives one atomicMax per pair: bit 63 = foreground and alpha > 0 (train.py:593-594: the background never hides an
 * object), bits 62..31 = alpha's bits made order-preserving, bits 30..0 = 0x7FFFFFFF - pair (equal alphas: the lowest
 * pair, i.e. the first object of the list).  A maximum does not depend on arrival order: bit-reproducible. */
int objnerf_mappoints_eval(const objnerf_net* net, int32_t K, int64_t N, int64_t M, const float* params, int64_t p_stride,
                           const float* scale, const float* pts, const float* boxes, const int32_t* info,
                           const int64_t* seg_off, const int32_t* pair_pt, float* pair_alpha, float* pair_color,
                           float* pair_hfeat, uint64_t* best, void* stream);
/* A wider object (the hidden-128 background, trainer.py:15): its segment of pair_pt is contiguous.  gather: out [n][3] =
 * pts [pair_pt [i]] - obj_center for the n entries at pair_pt (the caller passes pair_pt + seg_off [k]), the input of
 * objnerf_eval_points_ws; merge: the keys above for pairs pair0 .. pair0 + n - 1 from pair_alpha, into best. */
int objnerf_mappoints_gather(int64_t n, const int32_t* pair_pt, const float* pts, float obj_center, float* out, void* stream);
int objnerf_mappoints_merge(int64_t n, int64_t pair0, const int32_t* pair_pt, const float* pair_alpha, int32_t background,
                            uint64_t* best, void* stream);
/* best -> out_obj [N] int32 (position in the list; -1: no occupied candidate, trainer.py:71 occ > 0.5 <=> alpha > 0),
 * out_alpha [N] (the winner's; without one the largest candidate alpha, -inf without a candidate), optional out_pair [N]
 * int32 (the winning pair or -1) and out_color [N][3] (pair_color of the winner, 0 without one).  M = 0 (no pair at all:
 * best is all zero) is valid, pair_color may then be NULL: every point gets -1, -inf and colour 0. */
int objnerf_mappoints_resolve(int64_t N, int32_t K, int64_t M, const uint64_t* best, const int64_t* seg_off,
                              const float* pair_color, int32_t* out_obj, float* out_alpha, int32_t* out_pair,
                              float* out_color, void* stream);
/* out_clip (model.py:101) for the winners only: the winning pairs are compacted (they stay object-major), then
 * out_feat [point][C] = of_w . hfeat [pair] + of_b, once per winner; rows of points without a winner are NOT written (the
 * caller zeroes out_feat).  heads [K] (device): per object the head's weights of_w [C][H], of_b [C], the hidden rows
 * hfeat [..][H] with row (pair - row0), H a multiple of 32.  widths: the OBJNERF_MAPPOINTS_W* bits of the widths that
 * occur among the objects (one launch per bit; 32, 64 and 128 keep an object's weights in registers); an object whose
 * width's bit is missing gets no feature.  win_pair: 3 x min(N, M) int32 of scratch (winning pair, point, object). */
#define OBJNERF_MAPPOINTS_W32 1
#define OBJNERF_MAPPOINTS_W64 2
#define OBJNERF_MAPPOINTS_W128 4
#define OBJNERF_MAPPOINTS_WOTHER 8
typedef struct objnerf_mappoints_head_obj {
  const float* of_w; const float* of_b; const float* hfeat;
  int64_t row0;
  int32_t H, reserved;
} objnerf_mappoints_head_obj;
size_t objnerf_mappoints_head_workspace_bytes(int64_t M);
int objnerf_mappoints_head(int32_t K, int32_t C, int64_t N, int64_t M, const uint64_t* best, const int64_t* seg_off,
                           const int32_t* pair_pt, const objnerf_mappoints_head_obj* heads, int32_t widths, void* ws,
                           size_t ws_bytes, int32_t* win_pair, float* out_feat, void* stream);

/* Geometry evaluation of a map (objnerf_mapeval.hip; openobj_amd/map_eval.py): vMAP's accuracy / completion between
 * points sampled on two sets of meshes; the reference has no counterpart.  Added under ABI 14: the five entries below are
 * purely additive (no existing struct or signature changes), so OBJNERF_ABI_VERSION stays 14.
 *
 * objnerf_mesh_sample: N area-weighted points on the surfaces of S meshes stored back to back.  verts [V][3] fp64, faces
 * [F][3] int32 (global vertex rows), face_off / samp_off [S + 1] device int64 (segment s owns faces face_off[s] ..
 * face_off[s+1] and samples samp_off[s] .. samp_off[s+1]; samp_off[S] = N).  Per face area = 0.5 sqrt((cx cx + cy cy) +
 * cz cz) of c = (B - A) x (C - A) in fp64, amax the segment's exact maximum, q = (uint64) floor(area / amax * 2^32), the
 * exclusive integer prefix of q per segment, W its total (< 2^63).  Sample i of segment s: the Philox4x32-10 block of
 * counter (s, i, 0) on stream 8 under `seed` -> (x, y, z, w); t = mulhi64(x << 32 | y, W); the face k with prefix[k] <= t
 * < prefix[k+1] (a zero-area face is never drawn); u1 = u01(z), u2 = u01(w) widened to fp64, s = sqrt(u1),
 * p = ((1 - s) A + (s (1 - u2)) B) + (s u2) C per coordinate, every operation rounded on its own.  A draw depends on
 * (seed, s, i) only.  out_pts [N][3] fp64, out_tri [N] int32 = the global face row.  status (one int32, cleared here):
 * bit 0 a face names a vertex outside [0, V) (it counts as area 0), bit 1 a non-finite area (likewise), bit 2 a segment
 * asks for samples but has W == 0 (its samples are NaN, face -1).  ws: objnerf_mesh_sample_workspace_bytes(F, S).
 *
 * objnerf_nearest: for every query point of segment s (qry [nq][3] fp64 under q_off [S + 1]) the nearest point of
 * reference segment s (ref [nr][3] under r_off [S + 1]).  sorted_keys / perm: the reference's keys from objnerf_cell_keys
 * with seg_off = r_off, shift = 0 and side `cell`, sorted per segment (stable), perm[t] = the row at sorted position t;
 * mins [S][3] = that call's out_min.  out_d2 [nq] fp64 = the minimum over the segment of (dx dx + dy dy) + dz dz, every
 * operation rounded on its own; out_idx [nq] int64 = the SMALLEST row of ref that attains it; +inf and -1 for an empty
 * reference segment.  The result is exact for any cell > 0: cell only decides the speed.  Rings of cells around the
 * query's cell are searched until the best d^2 is strictly below (r cell)^2 (1 - 2^-20) or the rings cover the grid; a
 * query still open after ring max_rings is finished by brute force over its segment.  max_rings <= 0 selects the
 * built-in default, a compile-time constant taken from a measured sweep: pass 0.  Other values (at most 64) exist for
 * that sweep and for tests only -- the result never depends on it, and a large value makes a thread walk (2 r + 1)^2
 * columns per ring before it gives up.  status bit 0: a query is not finite (its outputs are +inf, -1).  ws: objnerf_nearest_workspace_bytes(nq, S).
 *
 * objnerf_seg_stats: out [S][5 + T] fp64 per segment of d [n] under off [S + 1]: the number of finite entries, of
 * non-finite ones, the sum, the sum of squares and the maximum (-inf without one) of the finite ones, and for each of
 * the T <= 4 thresholds (a HOST array) the number of finite d < threshold.  Thread-strided partial sums, then a fixed
 * tree: two calls write the same bytes. */
size_t objnerf_mesh_sample_workspace_bytes(int64_t F, int32_t S);
int objnerf_mesh_sample(int64_t V, int64_t F, int32_t S, int64_t N, const double* verts, const int32_t* faces,
                        const int64_t* face_off, const int64_t* samp_off, uint64_t seed, void* ws, size_t ws_bytes,
                        double* out_pts, int32_t* out_tri, int32_t* status, void* stream);
size_t objnerf_nearest_workspace_bytes(int64_t nq, int32_t S);
int objnerf_nearest(int64_t nr, int64_t nq, int32_t S, const double* ref, const int64_t* r_off, const int64_t* sorted_keys,
                    const int64_t* perm, const double* mins, double cell, const double* qry, const int64_t* q_off,
                    int32_t max_rings, void* ws, size_t ws_bytes, double* out_d2, int64_t* out_idx, int32_t* status,
                    void* stream);
int objnerf_seg_stats(int64_t n, int32_t S, const double* d, const int64_t* off, int32_t T, const double* thresholds,
                      double* out, void* stream);

/* Culling meshes to what the frames of a sequence observed (objnerf_meshcull.hip; openobj_amd/map_cull.py, DESIGN.md
 * 4.22): the step before accuracy / completion in vMAP's, iMAP's and NICE-SLAM's evaluations; the reference has no
 * counterpart.  Added under ABI 14: the four entries below are purely additive, so OBJNERF_ABI_VERSION stays 14.
 *
 * objnerf_vertex_views: views[v] += the number of frames of the batch that see vertex v (views [V] int32, in / out: the
 * caller zeroes it once and streams a sequence through in batches).  verts [V][3] fp64 world coordinates, t_cw [B][3][4]
 * fp64 = the upper 3 x 4 of inverse(T_WC) per frame (inverted by the caller), depth [B][W][H] fp32 metres, 0 = invalid.
 * Per vertex p and frame, in fp64, every operation rounded once and in this order, M = t_cw[f]:
 *   xc = ((M[0] px + M[1] py) + M[2] pz) + M[3]      (yc: M[4..7], zc: M[8..11])
 *   front  = zc > z_min
 *   u = (fx xc) / zc + cx,  v = (fy yc) / zc + cy,  iu = floor(u + 0.5),  iv = floor(v + 0.5)
 *   inside = front and margin <= iu <= W - 1 - margin and margin <= iv <= H - 1 - margin       (compared as doubles)
 *   seen   = inside and d > 0 and zc <= d + eps,  d = (double) depth[f][iu][iv]
 * A NaN or infinite coordinate makes every comparison false: the vertex is never seen and nothing is converted to an
 * integer or dereferenced before `inside` holds.  margin >= 0.  No atomics: a thread owns a vertex.
 *
 * objnerf_mesh_cull_count / _emit: the sub-mesh a vertex mask keeps.  keep_v [V] uint8 (non-zero = kept), faces [F][3]
 * int32.  A face stays iff all three (OBJNERF_CULL_ALL) or at least one (OBJNERF_CULL_ANY) of its corners are kept; the
 * output holds the kept faces in their original order and exactly the vertices those faces use, in ascending original
 * order (under ANY that includes corners that are not kept; a vertex no kept face uses is dropped under either rule).
 * A face that names a vertex outside [0, V) is never dereferenced: it is dropped and sets status bit 0.  Degenerate and
 * repeated faces pass through.  count: counts [2] int64 = (Vn, Fn) and status (one int32, cleared here), both on the
 * device; ws: objnerf_mesh_cull_workspace_bytes(V, F), handed on to emit unchanged.  emit (same V, F, rule, keep_v,
 * faces; Vn, Fn as counted): new_of_old [V] int32 (-1 = dropped), old_of_new [Vn] int32, faces_out [Fn][3] int32
 * re-indexed, face_old [Fn] int32 = the original row of each kept face.  Integers only, no atomics: two calls write the
 * same bytes. */
#define OBJNERF_CULL_ALL 0
#define OBJNERF_CULL_ANY 1
int objnerf_vertex_views(int64_t V, int32_t B, int32_t W, int32_t H, const double* verts, const double* t_cw,
                         const float* depth, double fx, double fy, double cx, double cy, double z_min, double eps,
                         int32_t margin, int32_t* views, void* stream);
size_t objnerf_mesh_cull_workspace_bytes(int64_t V, int64_t F);
int objnerf_mesh_cull_count(int64_t V, int64_t F, int32_t rule, const uint8_t* keep_v, const int32_t* faces, void* ws,
                            size_t ws_bytes, int64_t* counts, int32_t* status, void* stream);
int objnerf_mesh_cull_emit(int64_t V, int64_t F, int32_t rule, const uint8_t* keep_v, const int32_t* faces, const void* ws,
                           size_t ws_bytes, int64_t Vn, int64_t Fn, int32_t* new_of_old, int32_t* old_of_new,
                           int32_t* faces_out, int32_t* face_old, void* stream);

/* A novel view of the whole map in one launch chain (objnerf_mapview.hip; openobj_amd/map_view.py):
 * replaces the per-object loop of train.py:550-612 (`cfg.if_render`) -- one sceneObject.render_2D_syn (vmap.py:604-685)
 * per object and the z-buffer merge of train.py:581-598 on the host.  Added under ABI 14: the five entries below are
 * purely additive, so OBJNERF_ABI_VERSION stays 14.
 *
 * objnerf_view_rays_count / _emit (Trainer.sample_points_bbox, trainer.py:130-167, for every object at once): T_WC [4][4]
 * row-major, dirs_C [P][3] the camera rays of the view with p = w * H + h (the transposed [W, H] image), boxes [K][16] =
 * T_OC rows 0..2 [3][4] | extent / 2 [3] | unused, T_OC = inverse(T_WO) @ T_WC formed by the caller as
 * sample_points_bbox forms it.  Every (pixel, box) runs the arithmetic of objnerf_box_rays (one device function); the
 * hits of object k are segment k of a CSR in the caller's object order, ascending in p inside a segment (no atomics).
 * An object with at most one hit gets an empty segment (trainer.py:164-165).  count: seg_off [K + 1] int64 on the
 * device; ws: objnerf_view_rays_workspace_bytes(P, K), handed on to emit unchanged.  emit (same inputs; M = seg_off[K]
 * as counted, M >= 2^32 is EINVAL: the merge keys hold an entry in 32 bits): pix [M] int32, dirs_W [M][3], near [M]
 * (>= 0), far [M] (+ 0.2).
 *
 * objnerf_render_fwd_segmented: objnerf_render_fwd (fp32 mode, no feature hidden, no z) over the segments of every
 * hidden-32, n_freqs == 6 object of the view in ONE launch of persistent workgroups.  params / scale: the stacked arena
 * of those objects (row r at params + r * p_stride, scale[r]); origin [3]: the camera centre.  rows [n_rows][4] int64 on
 * the device: seg_lo, seg_hi (the row's entries of the CSR), u_lo (the row of u its first ray reads; < 0: drawn inside
 * the kernel under (seed, draw)), draw.  tiles [n_tiles][3] int32 on the device: arena row, first 16-ray group counted
 * from seg_lo, number of groups; a tile belongs to one row, tiles of a row are adjacent.  Ray r = entry - seg_lo is the
 * row of u and the Philox counter, as ray r of objnerf_render_fwd is: the outputs (CSR-aligned out_depth [M],
 * out_opacity [M], out_rgb [M][3]) are bit-equal to a per-object objnerf_render_fwd on the same rays, whatever
 * `workgroups` (0 = two per compute unit) is.  A row whose segment or draws would leave [0, M) / [0, u_rows) renders
 * nothing.
 *
 * objnerf_view_merge: the merge of train.py:581-598 in closed form.  info [K][2] int32: background flag, the id written
 * into the mask-id image.  An entry is offered iff !((depth < near) | (depth > far) | (opacity < 0.9)) and depth < 100;
 * W(p) = the offered foreground entry of smallest depth (ties: the earliest object), depth(p) = its depth or 100; the
 * painter of p is the last offered background entry behind W's object in the order with a smaller depth than W (without
 * W: the last one), otherwise W.  best_fg [P] uint64 and best_bg [P] uint32: workspace, initialised here.  Outputs per
 * pixel: out_rgb [P][3] uint8 (rgb * 255 truncated), out_maskid [P] int32 (0 = nothing painted), out_depth [P],
 * out_winner [P] int32 (the painter's entry, -1 = none).  64-bit atomicMin / 32-bit atomicMax of integers only: two
 * calls write the same bytes. */
size_t objnerf_view_rays_workspace_bytes(int64_t P, int32_t K);
int objnerf_view_rays_count(int64_t P, int32_t K, const float* T_WC, const float* boxes, const float* dirs_C, void* ws,
                            size_t ws_bytes, int64_t* seg_off, void* stream);
int objnerf_view_rays_emit(int64_t P, int32_t K, const float* T_WC, const float* boxes, const float* dirs_C, const void* ws,
                           size_t ws_bytes, int64_t M, int32_t* pix, float* dirs_W, float* near, float* far, void* stream);
int objnerf_render_fwd_segmented(const objnerf_net* net, int32_t n_rows, int64_t n_tiles, int32_t n_bins, int64_t M,
                                 const float* params, int64_t p_stride, const float* scale, const float* origin,
                                 const int64_t* rows, const int32_t* tiles, const float* dirs_W, const float* near,
                                 const float* far, const float* u, int64_t u_rows, uint64_t seed, float* out_depth,
                                 float* out_opacity, float* out_rgb, int32_t workgroups, void* stream);
int objnerf_view_merge(int64_t P, int32_t K, int64_t M, const int64_t* seg_off, const int32_t* pix, const float* depth,
                       const float* opacity, const float* rgb, const float* near, const float* far, const int32_t* info,
                       int32_t any_background, uint64_t* best_fg, uint32_t* best_bg, uint8_t* out_rgb, int32_t* out_maskid,
                       float* out_depth, int32_t* out_winner, void* stream);

/* Part features and open-vocabulary queries in a map view (objnerf_mapview.hip; MapView.query / .features, DESIGN.md
 * 4.24): sceneObject.render_2D_syn(render_part=True)'s render_partfeat (vmap.py:641-679) for the pixels of a merged view,
 * without the dense [P][512] image.  Added under ABI 14: the entries below are purely additive.
 *
 * objnerf_render_fwd_segmented_feat: objnerf_render_fwd_segmented plus out_hfeat [M][32], the composited feature hidden of
 * every rendered entry (CSR-aligned; the input of out_clip, model.py:100), bit-equal to objnerf_render_fwd's out_hfeat
 * per object; the other outputs are bit-equal to objnerf_render_fwd_segmented's.
 * objnerf_render_fwd_segmented_occupancy: the workgroups of that renderer (with_hfeat 0 / 1) the runtime places on one
 * compute unit; diagnostic.
 *
 * objnerf_view_query: for every painted pixel p (e = winner [p], an entry of object k) the part feature
 *   F = of_w_k . h_e + of_b_k * opacity [e]       (C channels; vmap.py:678: the linear head after compositing)
 * and against Q unit-length queries [Q][C]: out_sim [Q][P] = (queries [q] . F) / max(|F|, 1e-8) (objnerf_project's cosine
 * convention), out_label [P] = the first arg-max over q, out_best [P] = that maximum; any of the three may be NULL, all
 * three NULL skips the pass (queries may then be NULL; Q is still checked).  A pixel nothing painted, or whose painter no
 * head serves, gets NaN / -1.  With n_feat > 0: out_feat [n_feat][C] = F of pixel feat_pix [i] (int32), zeros for a pixel
 * out of [0, P), unpainted or unserved.  heads [K] on the device and heads_host [K], the same records in host memory (the
 * argument checks read these): per object of_w [C][H], of_b [C], hfeat = the composited hidden rows [n_rows][H] with row
 * (entry - row0); of_w, of_b and hfeat 16-byte aligned; hfeat NULL = this object serves nothing.  H a multiple of 32,
 * objects of different H in one call.  Every output location has one writer, the summation order is fixed by the MFMA
 * sequence: two calls write the same bytes, whatever `workgroups` (0 = four per compute unit) is.
 * EINVAL: Q < 1, Q > 16, M >= 2^32, an H that is no multiple of 32, a misaligned pointer.  ENOTSUP: an H other than 32,
 * 64, 128, C not a multiple of 16 or above 1020.  M = 0: only the unpainted fill (and zero rows). */
typedef struct objnerf_view_head_obj {
  const float* of_w; const float* of_b; const float* hfeat;
  int64_t row0, n_rows;
  int32_t H, reserved;
} objnerf_view_head_obj;
int objnerf_render_fwd_segmented_feat(const objnerf_net* net, int32_t n_rows, int64_t n_tiles, int32_t n_bins, int64_t M,
                                      const float* params, int64_t p_stride, const float* scale, const float* origin,
                                      const int64_t* rows, const int32_t* tiles, const float* dirs_W, const float* near,
                                      const float* far, const float* u, int64_t u_rows, uint64_t seed, float* out_depth,
                                      float* out_opacity, float* out_rgb, float* out_hfeat, int32_t workgroups,
                                      void* stream);
int objnerf_render_fwd_segmented_occupancy(int32_t with_hfeat);
int objnerf_view_query(int64_t P, int32_t K, int64_t M, int32_t C, int32_t Q, const int64_t* seg_off, const int32_t* pix,
                       const float* opacity, const int32_t* winner, const objnerf_view_head_obj* heads,
                       const objnerf_view_head_obj* heads_host, const float* queries, float* out_sim, int32_t* out_label,
                       float* out_best, int64_t n_feat, const int32_t* feat_pix, float* out_feat, int32_t workgroups,
                       void* stream);

/* The compact exported map (objnerf_partrows.hip; openobj_amd/query.py).  Added under ABI 14: the two
 * entries below are purely additive, so OBJNERF_ABI_VERSION stays 14.
 *
 * The unit part feature of a vertex, f^ = (W h + b) / max(|W h + b|, 1e-8) with h its feature hidden [H] and [W | b] its
 * object's out_clip head, is linear in the row  r = [h s, s],  s = 1 / max(|W h + b|, 1e-8):  f^ = A r,  A = [W | b]
 * ([C][H + 1], row-major).
 *
 * objnerf_part_rows: hfeat [V][hfeat_stride] (the first H floats of a row), of_w [C][H], of_b [C] -> rows
 * [V][row_stride_out]: r in the first H + 1 floats, zeros in floats H + 1 .. min(H + 4, row_stride_out) - 1, anything
 * beyond untouched.  W h + b runs on v_mfma_f32_16x16x4_f32 (the chain of objnerf_view_query), |.|^2 is summed in
 * registers; the C-wide vector is never written.  |W h + b| = 0 gives s = 1e8 and a finite row (the dense export's
 * f / |f| is NaN there).  row_stride_out >= H + 1, hfeat_stride >= H; 16-byte aligned pointers and strides that are
 * multiples of 4 take the 128-bit path, anything else the scalar one (same values).
 *
 * objnerf_part_expand: out [n][C] = A rows[index[i]] (index int64 [n] on the device; NULL: n == V, row i), zeros for an
 * index outside [0, V).  head [C][H + 1].
 *
 * Both: V = 0 (n = 0) is a no-op; every output location has one writer and the order of every sum is fixed: two calls
 * write the same bytes.  ENOTSUP: H not a multiple of 32 in 32 .. 256, C not a multiple of 16 in 16 .. 1024.  EINVAL: a
 * null pointer, a stride below the row width, n != V without an index. */
int objnerf_part_rows(int64_t V, int32_t H, int32_t C, const float* hfeat, int64_t hfeat_stride, const float* of_w,
                      const float* of_b, float* rows, int64_t row_stride_out, void* stream);
int objnerf_part_expand(int64_t V, int32_t H, int32_t C, const float* rows, int64_t row_stride, const float* head,
                        int64_t n, const int64_t* index, float* out, void* stream);

/* Scoring a rendered map view against a frame of the sequence (objnerf_vieweval.hip; openobj_amd/map_view_eval.py,
 * DESIGN.md 4.26); the reference writes the images (train.py:550-612) and compares nothing.  Added under ABI 14: the entry
 * below is purely additive, so OBJNERF_ABI_VERSION stays 14.
 *
 * objnerf_view_compare: one launch per frame.  Every image is [W][H], w-major (p = w * H + h).
 *   the rendered view: rgb_r u8 [W][H][3], depth_r f32, id_r i32, painted u8 [W][H] or NULL (= every pixel painted);
 *   the frame:         rgb_g u8 [W][H][3], depth_g f32 (metres, 0 = invalid), id_g i32;
 *   lut i32 [n_lut], G: an id i HAS ROW lut[i] iff 0 <= i < n_lut and 0 <= lut[i] < G; otherwise it has no row.
 * Outputs, all ADDED TO and never cleared (the caller zeroes them once per sequence, or once per frame):
 *   acc i64 [G + 1][9]: row r < G = the pixels whose id_g has row r, row G = every other pixel (column sums = the whole
 *   image).  Columns:
 *     0  pixels                              1  pixels with painted set
 *     2  sum over the 3 channels of (rgb_r - rgb_g)^2           3  the same over painted pixels only
 *     4  pixels with depth_g > 0             5  pixels with depth_g > 0 and depth_r < 100 (100: nothing wrote depth)
 *     6  sum over the pixels of column 5 of (int64) floor(e * 2^20), e = min(fabsf(depth_r - depth_g), 2^22): ONE fp32
 *        subtraction; the widening to fp64 and the scaling are exact (the clamp keeps an infinite depth_g defined)
 *     7  interior pixels                     8  sum over interior pixels of q         (both: SSIM below)
 *   conf i64 [G][G + 1] or NULL: for a pixel whose id_g has row r, column (row of id_r) is incremented, column G if id_r
 *   has no row -- the table of map_points.confusion (rows = ground truth, last column = prediction outside).
 *   ssim_map f32 [W][H] or NULL: per pixel the mean over the channels (`value` below, rounded to fp32), NaN outside the
 *   interior.
 *
 * SSIM (Wang et al. 2004: 11 x 11 Gaussian window, sigma 1.5, K1 0.01, K2 0.03, L 255, population covariance, per
 * channel), scored only where the whole window lies inside the image -- the INTERIOR 5 <= w < W - 5, 5 <= h < H - 5,
 * empty when W < 11 or H < 11 -- and made exact by integer taps that sum to 2^16:
 *     t = [67, 498, 2359, 7167, 13960, 17434, 13960, 7167, 2359, 498, 67]
 * (rint(65536 g) with the centre raised by one).  With x the rendered and y the frame's channel (u8):
 *   1-D pass:  sum t x, sum t y, sum t x^2, sum t y^2, sum t x y           (<= 65536 * 65025 < 2^32: uint32, exact)
 *   2-D:       Mx, My, Mxx, Myy, Mxy = sum t (1-D sums) over the other axis (< 2^48: integer, exact)
 * then ONE fixed sequence of fp64 operations, each rounded on its own (no contraction; C1 = 6.5025, C2 = 58.5225):
 *   mx = Mx * 2^-32, my = My * 2^-32, exx = Mxx * 2^-32, eyy = Myy * 2^-32, exy = Mxy * 2^-32          (all exact)
 *   mxmx = mx * mx,  mymy = my * my,  mxmy = mx * my
 *   vx = exx - mxmx, vy = eyy - mymy, cv = exy - mxmy
 *   a1 = (2 * mxmy) + C1,  a2 = (2 * cv) + C2,  b1 = (mxmx + mymy) + C1,  b2 = (vx + vy) + C2
 *   s  = (a1 * a2) / (b1 * b2)
 *   value = ((s_R + s_G) + s_B) / 3
 *   q = (int64) floor(value * 2^32)
 * Identical images give q = 2^32 exactly; an inverted image gives a negative q (floor rounds towards -inf).
 *
 * Every accumulated quantity is an integer: the tables do not depend on the order of summation, the grid (`workgroups`,
 * 0 = the default) or the path -- with G <= OBJNERF_VIEW_EVAL_LDS_ROWS a workgroup reduces into an LDS copy of the
 * tables and adds one 64-bit atomic per non-zero cell; above it, wave-aggregated global atomics.  Tiles are
 * OBJNERF_VIEW_EVAL_TILE pixels square.  The inputs are only read.
 * EINVAL: a null image, lut or acc, W or H < 1, W * H >= 2^31, G < 1 or > OBJNERF_VIEW_EVAL_MAX_ROWS, n_lut < 0. */
#define OBJNERF_VIEW_EVAL_TILE 32
#define OBJNERF_VIEW_EVAL_LDS_ROWS 64
#define OBJNERF_VIEW_EVAL_MAX_ROWS 32767
int objnerf_view_compare(int32_t W, int32_t H, const uint8_t* rgb_r, const float* depth_r, const int32_t* id_r,
                         const uint8_t* painted, const uint8_t* rgb_g, const float* depth_g, const int32_t* id_g,
                         const int32_t* lut, int32_t n_lut, int32_t G, int64_t* acc, int64_t* conf, float* ssim_map,
                         int32_t workgroups, void* stream);

/* Field gradients of the finished map: d alpha / d p, the nearest surface and the normal equations of a rigid alignment
 * (objnerf_mapalign.hip; openobj_amd/map_points.py, openobj_amd/map_align.py).  The reference has no
 * counterpart: it differentiates a network in its weights only.  Added under ABI 14: the entries below are purely
 * additive, so OBJNERF_ABI_VERSION stays 14.
 *
 * objnerf_mappoints_grad: the arguments of objnerf_mappoints_eval without best, colour and hfeat.  For every pair of the
 * hidden-32 objects (info as there) pair_alpha [M] = 10 * raw (model.py:88) and pair_grad [M][3] = d alpha / d p in world
 * units (the 1 / scale of embedding.py:47 included).  One fused launch on the tile walk of objnerf_mappoints_eval: the
 * density trunk forward, its four ReLU masks kept as bits, the chain backwards through the transposed weight reads.
 * Octaves 4 and 5 feed colour only and take no part.  A pair's arithmetic does not depend on its tile, its place in the
 * tile or the segment length: permuting the pairs permutes the outputs bit for bit.  ENOTSUP unless hidden = 32.
 *
 * objnerf_embed_bwd_pts: d_pts [K][N][3] of UniDirsEmbed.forward (embedding.py:46-55) from d_emb [K][N][129] and the
 * inputs of objnerf_embed: all six octaves and the three linear entries, one thread per point, no atomics.  With
 * objnerf_mlp_backward_ws it differentiates a network of any width in position (the layer-wise, slow path).
 *
 * objnerf_mapalign_select: d = alpha / max(|grad|, g_min) per pair, an estimate of the signed distance to the object's
 * zero level set (positive inside); one 64-bit atomicMin per pair into best [N], WHICH THE CALLER FILLS WITH ALL ONES
 * before the first select of a cloud.  Key: bits 62..31 the bits of |d| (a non-negative float's bit pattern is
 * order-preserving), bits 30..0 the pair; equal |d| goes to the lower pair.  A minimum does not depend on arrival order.
 * Launch it after every pair_alpha / pair_grad of the cloud is written.  g_min > 0.
 * objnerf_mapalign_resolve: best -> per point out_obj [N] int32 (position in the list, -1 for a point in no box), optional
 * out_pair [N] int32, out_d [N] (the signed d of the selected pair, +inf without one), out_alpha [N] and out_grad [N][3]
 * (the selected pair's, 0 without one).  M = 0 is valid (pair_alpha / pair_grad may then be NULL).
 *
 * objnerf_mapalign_transform: out [N][3] = float32(R p + t) for pts [N][3] fp32, t_rows = a HOST array of 12 doubles, the
 * rows of [R | t]; ((r0 x + r1 y) + r2 z) + t in fp64, every operation rounded on its own.
 *
 * objnerf_mapalign_accumulate: over the points with out_obj >= 0 and |d| <= tau, everything in fp64 from the fp32 values:
 * den = max(|grad|, g_min), d = alpha / den, n = grad / den, J = [(q - pivot) x n, n] (q = pts [n]); out [29] (device) =
 * the 21 upper entries of sum J J^T row by row, the 6 of sum J d, sum d^2, the inlier count.  pivot: a HOST array of 3.
 * A workgroup owns 1024 consecutive points; its partial sums go to ws (objnerf_mapalign_workspace_bytes(N)) and a second
 * launch adds them: the order of every sum depends on N alone, two calls write the same bytes.  Nothing is allocated. */
int objnerf_mappoints_grad(const objnerf_net* net, int32_t K, int64_t N, int64_t M, const float* params, int64_t p_stride,
                           const float* scale, const float* pts, const float* boxes, const int32_t* info,
                           const int64_t* seg_off, const int32_t* pair_pt, float* pair_alpha, float* pair_grad,
                           void* stream);
int objnerf_embed_bwd_pts(const objnerf_net* net, int32_t K, int64_t N, const float* params, int64_t p_stride,
                          const float* scale, const float* pts, const float* d_emb, float* d_pts, void* stream);
int objnerf_mapalign_select(int64_t N, int64_t M, const int32_t* pair_pt, const float* pair_alpha, const float* pair_grad,
                            float g_min, uint64_t* best, void* stream);
int objnerf_mapalign_resolve(int64_t N, int32_t K, int64_t M, const uint64_t* best, const int64_t* seg_off,
                             const float* pair_alpha, const float* pair_grad, float g_min, int32_t* out_obj,
                             int32_t* out_pair, float* out_d, float* out_alpha, float* out_grad, void* stream);
int objnerf_mapalign_transform(int64_t N, const float* pts, const double* t_rows, float* out, void* stream);
size_t objnerf_mapalign_workspace_bytes(int64_t N);
int objnerf_mapalign_accumulate(int64_t N, const float* pts, const int32_t* obj, const float* alpha, const float* grad,
                                const double* pivot, double tau, double g_min, void* ws, size_t ws_bytes, double* out,
                                void* stream);

/* The mask front end: the image work of the reference's maskclustering/mask_gen.py between its four models
 * (objnerf_maskprep.hip; openobj_amd/mask_prep.py).  Added under ABI 14: the entries below are purely
 * additive, so OBJNERF_ABI_VERSION stays 14.  Painting the id image (mask_gen.py:289-295) is objnerf_part_index on the
 * rank-permuted masks.  1 <= F <= 65535 frames, 1 <= H, W <= 32767 (a squared pixel distance fits 31 bits).
 *
 * objnerf_cc_label (split_mask's cv2.connectedComponentsWithStats, :168, for every mask of F frames at once):
 * ids [F][H][W] int32 -> label [F][H][W] int32, 8-connectivity between pixels of EQUAL non-zero id; the label is the flat
 * index y * W + x inside the frame of the component's first pixel in raster order, -1 where the id is 0.  Union-find over
 * 32 x 32 tiles in LDS, a merge of the tile borders, a flatten: the root of a component is its smallest index whatever
 * the order of the unions, so two calls write the same bytes.
 *
 * objnerf_cc_table: the components of every frame in raster order of their first pixel.  comp_off [F + 1] int64 (device),
 * table [cap][8] int32 rows {first pixel, id, area, x0, y0, x1, y1, frame} (x0 / y0 the smallest column / row, x1 / y1
 * the largest plus one: min_rect_bbox, :125-137), slot [F][H][W] int32 = the row of a component at its first pixel (-1
 * elsewhere).  The order comes from count / scan / emit without atomics; area and box are integer atomics.  Rows past
 * cap are not written: the caller compares comp_off [F] with cap and calls again with a larger one.
 * ws: objnerf_cc_table_workspace_bytes(F, H, W).
 *
 * objnerf_cc_boundary: sel [rows] int32 maps a table row to a list s in [0, S) or -1.  boff [S + 1] int32 = the CSR
 * offsets of the lists, bpix [bcap] uint32 = (y << 16) | x of the pixels of the selected components that have a
 * 4-neighbour outside the component; cursor [S] int32 is scratch.  The order INSIDE a list is whatever the atomics give:
 * only order-free reductions may read it.  Entries past bcap are dropped: bcap >= the selected components' areas holds all.
 *
 * objnerf_cc_gaps (closest_distance, :139-160, without its random tenth): pairs [P][2] int32 of lists -> d2 [P] int32,
 * the exact minimum squared Euclidean distance between the two pixel sets (the closest pair lies on the boundaries).
 * Brute force over LDS tiles of the second list, one atomicMin per workgroup; INT32_MAX for an empty list.
 *
 * objnerf_cc_relabel (:334-349): final_id [rows] int32 = the id each component ends with (0 = dropped) -> out_ids
 * [F][H][W] int32 and stats [F][256][8] int32 rows in the table's layout (area, box of every final id; final ids lie in
 * [0, 256), others are written as 0).
 *
 * objnerf_clip_crops (:495-516, CLIP's preprocessing of the padded crops): image [H][W][3] uint8, n crops.  PIL's two-pass
 * integer bicubic resample (ImagingResample: horizontal first into a uint8 intermediate, clip8((2^21 + sum) >> 22) a pass)
 * with the caller's coefficient tables, for the 224 x 224 pixels the centre crop keeps; then v / 255.0f, (x - mean) / std
 * in fp32 -> out [n][3][224][224], channel c of the output = channel c of the image.
 *   desc [n][8] int32  x0, y0 (the crop's origin in the image), w, h, row0, nrows (the crop rows the vertical pass reads:
 *                      the intermediate's rows), hcopy, vcopy (>= 0: that pass is skipped, output column / row o is crop
 *                      column / row hcopy + o / vcopy + o; -1: resample)
 *   hb [n][224][2], hk [n][224][kh]   per kept output column: first crop column and count (<= kh), 22-bit coefficients
 *   vb, vk (kv)                       the same for the kept output rows
 *   tmp [n][tmp_rows][224][3] uint8   the intermediate, tmp_rows >= every nrows
 * Every index is clamped into the image, the tables and tmp. */
size_t objnerf_cc_table_workspace_bytes(int32_t F, int32_t H, int32_t W);
int objnerf_cc_label(int32_t F, int32_t H, int32_t W, const int32_t* ids, int32_t* label, void* stream);
int objnerf_cc_table(int32_t F, int32_t H, int32_t W, const int32_t* ids, const int32_t* label, void* ws, size_t ws_bytes,
                     int64_t cap, int64_t* comp_off, int32_t* table, int32_t* slot, void* stream);
int objnerf_cc_boundary(int32_t F, int32_t H, int32_t W, const int32_t* label, const int32_t* slot, const int32_t* sel,
                        int64_t rows, int32_t S, int32_t* boff, int32_t* cursor, uint32_t* bpix, int64_t bcap,
                        void* stream);
int objnerf_cc_gaps(int32_t P, const int32_t* pairs, int32_t S, const int32_t* boff, const uint32_t* bpix, int64_t bcap,
                    int32_t* d2, void* stream);
int objnerf_cc_relabel(int32_t F, int32_t H, int32_t W, const int32_t* label, const int32_t* slot, const int32_t* final_id,
                       int64_t rows, int32_t* out_ids, int32_t* stats, void* stream);
#define OBJNERF_CLIP_SIDE 224
int objnerf_clip_crops(int32_t n, int32_t H, int32_t W, const uint8_t* image, const int32_t* desc, int32_t kh,
                       const int32_t* hb, const int32_t* hk, int32_t kv, const int32_t* vb, const int32_t* vk,
                       int32_t tmp_rows, uint8_t* tmp, float* out, void* stream);

/* A navigation volume of the map (objnerf_mapvolume.hip; openobj_amd/map_volume.py).  Added under ABI 14:
 * the entries below are purely additive, so OBJNERF_ABI_VERSION stays 14.  A grid of nx x ny x nz voxels, every axis in
 * [1, 1024] and at most 2^31 - 1 voxels (EINVAL otherwise), idx = (z * ny + y) * nx + x; label [nz][ny][nx] int32, a voxel
 * is OCCUPIED iff label >= 0.  All volume data is integer, every reduction a minimum over keys that no two candidates
 * share: two calls write the same bytes.  Nothing is allocated.
 *
 * objnerf_volume_centres: out [nzs][ny][nx][3] fp32, the centres of the z-planes [z0, z0 + nzs): per component
 * origin + (float(i) + 0.5f) * voxel, one fp32 multiply and one fp32 add.  origin: a HOST array of 3 floats.
 *
 * objnerf_volume_project: the axis (0 = x, 1 = y, 2 = z) collapsed to length 1: out = the label of the occupied voxel with
 * the lowest index along the axis in every column, -1 for a column without one.
 *
 * objnerf_volume_clearance: dist2 [nz][ny][nx] int32 = the smallest dx^2 + dy^2 + dz^2 (voxel units) to an occupied voxel,
 * site = the linear index of the occupied voxel at that distance, the LOWEST index among several; an occupied voxel has
 * 0 and its own index; without an occupied voxel anywhere INT32_MAX and -1.  Three passes, x, y, z, each the
 * lexicographic minimum of (partial dist2, site) over the line; tmp_dist2 / tmp_site: two more volumes, the middle pass's
 * output (distinct from dist2 / site).
 *
 * objnerf_volume_reach_rounds: n_rounds relaxation rounds of the 26-connected path cost (weights 3 / 4 / 5 for a face /
 * edge / corner move) through TRAVERSABLE voxels, label < 0 and dist2 >= r2.  cost [nz][ny][nx] uint32, 0xFFFFFFFF =
 * not reached: the caller fills it, writes 0 at the start voxel and 1 at the start voxel's tile in active [2][T] int32
 * (T = objnerf_volume_reach_tiles, tiles of 8 x 8 x 8, tile index (tz * nty + ty) * ntx + tx; all else 0) before round 0.
 * Round round0 + r reads active [(round0 + r) & 1], clears what it read, flags in the other half the tiles whose halo it
 * changed, and writes 1 to changed [r] (zeroed by the caller) iff it lowered a cost.  A round that lowers nothing is the
 * last: every later one is empty.  No workgroup waits for another and every in-kernel loop is bounded by the tile size.
 * The caller keeps 5 x (traversable voxels) below 2^32 - 6, so that no cost can wrap.
 *
 * objnerf_volume_goals: table [K] uint64, FILLED WITH ALL ONES by the caller; a traversable voxel u with a finite cost
 * offers dist2 [u] << 32 | u to row label [site [u]]: the row's minimum is the reachable voxel that comes closest to the
 * object, the lowest index among equals.
 *
 * objnerf_volume_paths: G goal voxels -> out [G][cap] int32, the voxels from the goal back to the start, and len [G]: the
 * number of voxels, NEGATIVE when it exceeds cap (nothing is written past cap), 0 for a goal outside the grid, not
 * traversable or not reached.  The predecessor of u is the first neighbour v in the order (dz, dy, dx) over {-1, 0, 1}^3,
 * dz slowest, the centre left out, that lies in the grid, is traversable and has cost [v] + w(v, u) == cost [u]; at most
 * cost [goal] / 3 + 1 steps. */
int objnerf_volume_centres(int32_t nx, int32_t ny, int32_t nz, int32_t z0, int32_t nzs, const float* origin, float voxel,
                           float* out, void* stream);
int objnerf_volume_project(int32_t nx, int32_t ny, int32_t nz, int32_t axis, const int32_t* label, int32_t* out,
                           void* stream);
int objnerf_volume_clearance(int32_t nx, int32_t ny, int32_t nz, const int32_t* label, int32_t* dist2, int32_t* site,
                             int32_t* tmp_dist2, int32_t* tmp_site, void* stream);
int64_t objnerf_volume_reach_tiles(int32_t nx, int32_t ny, int32_t nz);
int objnerf_volume_reach_rounds(int32_t nx, int32_t ny, int32_t nz, const int32_t* label, const int32_t* dist2, int32_t r2,
                                uint32_t* cost, int32_t* active, int32_t round0, int32_t n_rounds, int32_t* changed,
                                void* stream);
int objnerf_volume_goals(int32_t nx, int32_t ny, int32_t nz, int32_t K, const int32_t* label, const int32_t* dist2,
                         const int32_t* site, const uint32_t* cost, int32_t r2, uint64_t* table, void* stream);
int objnerf_volume_paths(int32_t nx, int32_t ny, int32_t nz, const int32_t* label, const int32_t* dist2, int32_t r2,
                         const uint32_t* cost, int32_t G, const int32_t* goals, int32_t cap, int32_t* out, int32_t* len,
                         void* stream);

/* Part regions: the connected surface patches of a part query on the map's meshes, with pose (objnerf_mapregions.hip;
 * openobj_amd/map_regions.py).  Added under ABI 14: the entries below are purely additive, so
 * OBJNERF_ABI_VERSION stays 14.  The whole map in one call: S objects, verts fp64 [V][3] in packed map order with
 * vert_off [S + 1] int64, faces int32 [F][3] of PACKED vertex ids with face_off [S + 1] int64 (face f belongs to the
 * object whose range holds f), sims fp32 [V][Q] and a column q, thr fp32 [S].  1 <= V <= 2^31 - 1, 0 <= F <= 2^31 - 1,
 * 1 <= S <= 65535, 1 <= Q <= 16, 0 <= q < Q; EINVAL otherwise, for a null pointer and for a short workspace, before any
 * launch.  Nothing is allocated.  status: one int32 the caller zeroes; bits are OR-ed in.
 *
 * SELECTION: vertex v of object s is selected iff sims[v][q] >= thr[s], one fp32 compare: a NaN on either side selects
 * nothing.  CONNECTION: two selected vertices are connected iff some face names both.  A face that names a vertex
 * outside [0, V) raises status bit 0, one that names a vertex outside its own object's range raises bit 1; either joins
 * nothing, contributes nothing, and nothing is read through its ids.  A face with a repeated vertex or zero area is
 * legal: it joins its vertices and adds zero area.
 *
 * objnerf_regions_label: root [V] int32 = the smallest packed index of the vertex's region, -1 for a vertex that is not
 * selected (union-find whose parent is always a smaller index, one thread per face, then a flatten: the result does not
 * depend on the order of the unions).  The roots are compacted per object in ascending vertex order by count / scan /
 * emit without atomics: reg_off [S + 1] int64 (device; R = reg_off [S] is the number of regions) and label [V] int32 =
 * the row of the vertex's region, -1 where not selected.  vmax: the largest vertex count of an object (1 <= vmax <= V),
 * the extent of the compaction's grid: a vertex past vmax inside its object is never found as a root.
 * ws: objnerf_regions_workspace_bytes(V, F, S) (0: sizes out of range).
 *
 * objnerf_regions_table: table int64 [R][OBJNERF_REGION_ROW], every entry the result of integer atomics (or a function of
 * such entries), so any schedule gives the same bytes.  Columns:
 *    0 root   1 object   2 vertices   3 faces   4 area_q   5..7 first moments   8..10 normal   11..13 box minimum
 *   14..16 box maximum   17 peak   18..20 centroid   21..26 second moments xx, xy, xz, yy, yz, zz
 *   27..29 residual first moments   30..31 zero
 * box: per axis the minimum / maximum of key(fp32(coordinate)), key(x) = bits ^ 0xFFFFFFFF for a set sign bit, else
 * bits | 0x80000000 (unsigned order = float order).  peak: the maximum of key(sim) << 32 | (~v & 0xFFFFFFFF) as an
 * unsigned 64-bit number: the selected vertex of the highest similarity, the smallest index among equals.
 * A face contributes iff all three of its vertices are selected (they are then in one region).  With a = the first
 * vertex of the face's object (the anchor), A, B, C its vertices, every fp64 operation rounded on its own:
 *    dA = A - a, dB = B - a, dC = C - a
 *    c = (dB - dA) x (dC - dA)              each component u_j w_k - u_k w_j: two products, one difference
 *    area = 0.5 sqrt((cx cx + cy cy) + cz cz)
 *    s = (dA + dB) + dC
 *    area_q           += q44(area)
 *    first moment j   += q44((area s_j) / 3)
 *    normal j         += q44(0.5 c_j)
 * q44(x) = llrint(x 2^44) (nearest, ties to even); a NaN, an infinity or |x 2^44| >= 2^62 counts as 0 and raises status
 * bit 2.  centroid j (the bits of an fp64, relative to the anchor) = double(first moment j) / double(area_q), 0.0 when
 * area_q <= 0.  Then, with e_i = d_i - centroid (i = A, B, C) and t = (e_A + e_B) + e_C,
 *    second moment jk += q44((area (((e_Aj e_Ak + e_Bj e_Bk) + e_Cj e_Ck) + t_j t_k)) / 12)
 *    residual j       += q44((area t_j) / 3)
 * The second moment is the exact integral of (x - centroid)_j (x - centroid)_k over the triangle before rounding.  The
 * residual is the first moment about the centroid column: what the roundings of pass A and of the division left over.
 * A reader refines the centroid to anchor + centroid + residual / area_q; its error is then one rounding of 2^-45 per
 * face divided by the area, however far the region lies from the anchor.
 * Inside a wave, runs of neighbouring lanes with the same row are folded by a segmented scan and the last lane of a run
 * issues the atomics. */
#define OBJNERF_REGION_ROW 32
size_t objnerf_regions_workspace_bytes(int64_t V, int64_t F, int32_t S);
int objnerf_regions_label(int64_t V, int64_t F, int32_t S, int64_t vmax, int32_t Q, int32_t q, const int64_t* vert_off,
                          const int64_t* face_off, const int32_t* faces, const float* sims, const float* thr, void* ws,
                          size_t ws_bytes, int32_t* root, int32_t* label, int64_t* reg_off, int32_t* status, void* stream);
int objnerf_regions_table(int64_t V, int64_t F, int32_t S, int32_t Q, int32_t q, const int64_t* vert_off,
                          const int64_t* face_off, const double* verts, const int32_t* faces, const float* sims,
                          const int32_t* root, const int32_t* label, int64_t R, int64_t* table, int32_t* status,
                          void* stream);

/* A rasteriser for the map's meshes: one view of the exported map, whatever colours its vertices carry
 * (objnerf_mapraster.hip; openobj_amd/map_raster.py).  Added under ABI 14: the entries below are purely
 * additive, so OBJNERF_ABI_VERSION stays 14.  The map as the part regions take it: verts fp64 [V][3], faces int32 [F][3]
 * of PACKED vertex ids, face_off int64 [S + 1] (face f belongs to the object whose range holds f), plus hide uint8 [S],
 * ids int32 [S] (the value of the mask-id image), t_cw fp64 [3][4] on the device = the upper rows of inverse(T_WC),
 * inverted by the caller in fp64.  Images are [W][H], w-major (p = w H + h).  0 <= V, F <= 2^31 - 1, 0 <= S <= 65535
 * (F > 0 needs V, S >= 1), 1 <= W, H <= 65536, W H <= 2^31 - 1, z_near > 0; EINVAL otherwise, for a null pointer and for
 * a short workspace, before any launch.  Nothing is allocated.  The result is THESE BYTES, whatever the kernels do:
 *
 * VERTEX p, in fp64, every operation rounded once, M = t_cw:
 *    xc = ((M[0] px + M[1] py) + M[2] pz) + M[3]            (yc: M[4..7], zc: M[8..11]; objnerf_vertex_views' sequence)
 *    u = (fx xc) / zc + cx,   v = (fy yc) / zc + cy
 *    X = floor(u 256 + 0.5),  Y = floor(v 256 + 0.5)
 *    ok = zc >= z_near and |X| <= 2^25 and |Y| <= 2^25     (compared as doubles, before any conversion; a NaN: not ok)
 *    iz = 1 / zc
 * A vertex that fails zc >= z_near is dropped "by z_near", one that passes it and fails the bound "by the bound".  The
 * sample point of pixel (i, j) is (256 i, 256 j).
 * FACE f of object s is drawn iff its three ids lie in [0, V) (else status bit 0 is raised and nothing is read through
 * them), hide[s] == 0, its three vertices are ok (no near-plane clipping), and
 *    A = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) != 0                                                          (int64)
 * If A < 0, corners 1 and 2 are swapped (both sides are drawn) and A = -A.  With E(a, b, P) = (bx - ax)(Py - ay) -
 * (by - ay)(Px - ax):  w0 = E(v1, v2, P), w1 = E(v2, v0, P), w2 = E(v0, v1, P); pixel P is covered iff w0, w1, w2 >= 0
 * (no top-left rule: a pixel on a shared edge is covered by both faces and the key decides).  Every w is below 2^53, so
 * (double) w is exact.
 *    q = ((w0 iz0) + (w1 iz1)) + (w2 iz2),   z = (double) A / q,   d = (float) z
 *    key = (uint64(bits(d)) << 32) | f
 * key [W][H] holds the minimum key per pixel, all ones where nothing is drawn: the nearest face, the lowest face id at
 * equal fp32 depth.
 * stats int64 [8]: every face adds one to exactly one counter, the first of this list that applies:
 *    6 a bad index   7 hidden   3 a corner dropped by z_near   4 a corner dropped by the bound   5 degenerate (A = 0)
 *    2 without any sample (the box of the face, clipped to the screen, holds no sample point)
 *    0 drawn on the small path (the clipped box is at most small_box pixels wide and high)   1 drawn on the large path
 * small_box: a private knob as the _workgroups arguments are (negative: the default, 4; 0: every face takes the large
 * path; INT32_MAX: every face the small one): the images do not depend on it, only counters 0 and 1.
 *
 * objnerf_raster_visibility: ws [objnerf_raster_workspace_bytes(V, F)] (0: sizes out of range) -> key, stats (both
 * cleared here) and status (one int32 the caller zeroes; bits are OR-ed in); ws then holds the vertex records that
 * objnerf_raster_resolve reads.  Launches: vertices, faces (small faces in the thread; the others appended to a list),
 * the list (its length read on the device by a fixed grid).  64-bit integer atomicMin / atomicAdd only.
 * passes: 0 for a caller.  DIAGNOSTIC, for tools/raster_bench.py: a bit mask of the launches to run on what an earlier
 * whole call left in ws (1: vertices; 2: the clears and the faces; 4: the list), so that each can be timed.
 *
 * objnerf_raster_resolve (same V, F, S, W, H, verts, faces, face_off, ws, key): per pixel with a key, face = the low
 * 32 bits, winner = s, maskid = ids[s], depth = d, and with t_k = w_k iz_k (the products of q)
 *    vertex = the packed id of the corner with the largest t_k (fp64; a tie: the first corner in the swapped order)
 *    b_k = t_k / q,   c = ((b0 c0) + (b1 c1)) + (b2 c2)    per channel, c_k = (double) colors[corner k] (fp32 [V][3])
 *    shading = 1:  c = c shade,  shade = ambient + (1 - ambient) (|n . g| / (|n| |g|)),  e1 = p1 - p0, e2 = p2 - p0,
 *                  n = e1 x e2 (each component two products, one difference), g = ((p0 + p1) + p2) / 3 - cam,
 *                  n . g = (nx gx + ny gy) + nz gz, |x| = sqrt((xx xx + xy xy) + xz xz); the corners in the face's OWN
 *                  order, world coordinates; shade = 1 where |n| |g| is not > 0
 *    rgb = floor(clamp(c, 0, 1) 255 + 0.5)                  (a NaN counts as 0)
 * A pixel without a key: winner -1, maskid 0, depth 100, face -1, vertex -1, rgb = background (0xRRGGBB).
 * counts int64 [S] (cleared here): the pixels each object wins, integer adds.  0 <= ambient <= 1. */
size_t objnerf_raster_workspace_bytes(int64_t V, int64_t F);
int objnerf_raster_visibility(int64_t V, int64_t F, int32_t S, int32_t W, int32_t H, const double* verts,
                              const int32_t* faces, const int64_t* face_off, const uint8_t* hide, const double* t_cw,
                              double fx, double fy, double cx, double cy, double z_near, int32_t small_box,
                              int32_t passes, void* ws, size_t ws_bytes, uint64_t* key, int64_t* stats, int32_t* status, void* stream);
int objnerf_raster_resolve(int64_t V, int64_t F, int32_t S, int32_t W, int32_t H, const double* verts,
                           const int32_t* faces, const int64_t* face_off, const int32_t* ids, const float* colors,
                           const void* ws, size_t ws_bytes, const uint64_t* key, double cam_x, double cam_y, double cam_z,
                           double ambient, int32_t shading, int32_t background, uint8_t* rgb, int32_t* maskid, float* depth,
                           int32_t* winner, int32_t* face, int32_t* vertex, int64_t* counts, void* stream);

/* Ray casting over the map's meshes: first hit and line of sight (objnerf_maprays.hip; openobj_amd/map_rays.py,
 * DESIGN.md 4.32).  Added under ABI 14: the entries below are purely additive, so OBJNERF_ABI_VERSION stays 14.  The
 * mesh as the rasteriser takes it (verts fp64 [V][3], faces int32 [F][3], face_off int64 [S + 1], hide uint8 [S], ids
 * int32 [S]; the same size limits), rays o, d fp64 [N][3] (d is NOT normalised; t is in units of d), 0 <= N <= 2^31 - 1,
 * a window t_min >= 0 and t_max (scalars, or one per ray where t_min_ray / t_max_ray are not null; a per-ray t_min is the
 * caller's to keep >= 0), pad >= 0 fp64, leaf >= 1 (negative: the default, 4; an ASSUMED value).  EINVAL for sizes out of
 * range, a null pointer and a short workspace, before any launch.  Nothing is allocated.
 *
 * THE RESULT IS DEFINED WITHOUT THE HIERARCHY.  Every operation rounds once in fp64 (no contraction); a dot product is
 * (a0 b0 + a1 b1) + a2 b2; a cross product a x b has the components a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0 (two
 * products, one difference).
 * RAY:   inv_k = 1 / d_k; axis k is PARALLEL iff inv_k is not finite.  A ray with a component of o or d that is not
 *        finite, or with d = 0, hits nothing, raises status bit 1 and is counted.
 * SLAB TEST of a box [lo, hi]: tn = -inf, tf = +inf; on a parallel axis the box passes iff lo_k <= o_k <= hi_k; on
 *        another a = (lo_k - o_k) inv_k, b = (hi_k - o_k) inv_k, tn = max(tn, min(a, b)), tf = min(tf, max(a, b)).  The
 *        box passes iff tn <= tf, tf >= t_min and tn <= t_max.
 * FACE f of object s IS HIT iff
 *    (a) its three ids lie in [0, V) (else it is never hit and status bit 0 is raised), its three corners are finite,
 *        and hide[s] == 0;
 *    (b) its own box passes the slab test, lo = min of the corners - pad, hi = max of the corners + pad, giving tn_f;
 *    (c) e1 = p1 - p0, e2 = p2 - p0, pv = d x e2, det = e1 . pv, det == 0 or NaN: a miss; tv = o - p0, qv = tv x e1,
 *        U = tv . pv, Vv = d . qv, T = e2 . qv; if det < 0 all four are negated (both sides are hit); accepted iff
 *        U >= 0, Vv >= 0 and U + Vv <= det;
 *    (d) t = T / det + 0.0 (the sum turns -0 into +0) satisfies t_min <= t <= t_max and tn_f <= t.
 * KEY:   key = (uint64(bits((float) t)) << 32) | f; a ray's result is the MINIMUM key over the hit faces, all ones where
 *        there is none: the nearest face and, at equal fp32 t, the lowest face id.
 * Gates (b) and (d) make a hierarchy harmless by the monotonicity of IEEE rounding alone: a node's box contains its
 * faces' boxes, so under the same sequence its tn is <= and its tf is >= theirs; a node that fails the slab test holds
 * no hit, and one with (float) tn > (float) t of the best key so far (strictly, as fp32) holds no smaller key.  Node
 * boxes are fp32, rounded outward.  Moeller-Trumbore in floating point is not watertight: a ray exactly through a shared
 * edge may in principle miss both neighbours.
 *
 * objnerf_rays_workspace_bytes(F, leaf): 0 for sizes out of range.  The workspace holds, from its start, the nodes
 * (32 bytes each: lo [3], hi [3] fp32, the split axis, 0; 2 P of them in heap order, children 2 n and 2 n + 1, node 0
 * unused, P = the power of two >= ceil(F / leaf), leaf i = node P + i; rounded up to 256 bytes) and then one slot per
 * sorted face {int32 face (-1: never hit), int32 object}.
 * objnerf_rays_build, stage 1: codes int64 [F] = the 63-bit Morton code (21 bits an axis, x highest) of the centre of the
 * face's padded box inside the scene box [lo, hi] the caller passes (any box: it only shapes the tree), INT64_MAX for a
 * face that fails (a) but for hide.  The caller sorts the codes STABLY and passes the permutation as `order` to
 * stage 2: the slots, the leaves' boxes and the levels above them, bottom up, one launch a level, no atomics; every byte
 * of the nodes and the slots is written, the same bytes in every run.  status: one int32 the caller zeroes; bit 0 is
 * OR-ed in by either stage.  hide takes no part: changing it needs no rebuild.
 * objnerf_rays_cast (same V, F, S, leaf, verts, faces, pad as the build): mode bit 0 = ANY-HIT (hit uint8 [N] = whether
 * a key exists; the walk stops at the first hit found; key may be null), else key uint64 [N] (hit may be null); mode
 * bit 1 = visit the children in fixed order with the stackless successor (n + 1) >> ctz(n + 1) instead of the nearer
 * child first (a 64-bit trail in registers): the results do not depend on it.  stats int64 [5] (cleared here): rays, hits,
 * bad rays, node visits, face tests (the last two: diagnostics that depend on mode and leaf).  status: bit 1 is OR-ed in.
 * objnerf_rays_resolve (same mesh and rays, the keys of a first-hit cast): per ray with a key, recomputed on the winning
 * face: hit = 1, face, winner = the object (a search of face_off), maskid = ids[winner], t = the fp32 of the key,
 *    bary = (u, v) = (U / det, Vv / det) fp64,   point_k = o_k + t d_k with the fp64 t of (d),
 *    normal = e1 x e2, negated where det was negative (unnormalised, facing the origin of the ray),
 *    vertex = the packed id of the corner with the largest of ((1 - u) - v, u, v), the first at a tie.
 * Without a key: hit 0, face = winner = vertex = -1, maskid 0, t = +inf, bary, point and normal = NaN
 * (0x7ff8000000000000). */
size_t objnerf_rays_workspace_bytes(int64_t F, int32_t leaf);
int objnerf_rays_build(int32_t stage, int64_t V, int64_t F, int32_t S, int32_t leaf, const double* verts, const int32_t* faces,
                       const int64_t* face_off, double pad, double lo_x, double lo_y, double lo_z, double hi_x, double hi_y,
                       double hi_z, int64_t* codes, const int64_t* order, void* ws, size_t ws_bytes, int32_t* status,
                       void* stream);
int objnerf_rays_cast(int32_t mode, int64_t V, int64_t F, int32_t S, int32_t leaf, int64_t N, const double* verts,
                      const int32_t* faces, const uint8_t* hide, const void* ws, size_t ws_bytes, double pad, const double* o,
                      const double* d, double t_min, double t_max, const double* t_min_ray, const double* t_max_ray,
                      uint64_t* key, uint8_t* hit, int64_t* stats, int32_t* status, void* stream);
int objnerf_rays_resolve(int64_t V, int64_t F, int32_t S, int64_t N, const double* verts, const int32_t* faces,
                         const int64_t* face_off, const int32_t* ids, const double* o, const double* d, const uint64_t* key,
                         uint8_t* hit, float* t, int32_t* face, int32_t* winner, int32_t* maskid, int32_t* vertex, double* bary,
                         double* point, double* normal, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OBJNERF_HIP_H */
