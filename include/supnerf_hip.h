/*
 * supnerf_hip.h -- C ABI of libsupnerf_hip.so: the MI355X (gfx950) implementation of
 * SUP-NeRF's volumetric rendering hot path.
 *
 * The reference (abhi1kumar/SUP-NeRF) has no FFI/plugin layer: its callers bind ordinary
 * Python functions by name.  The entry points below are therefore
 * what a ctypes/cffi stub inside the reference's src/utils.py, src/renderer.py and
 * src/model_supnerf.py would bind to replace the bodies of those functions; each one cites
 * the reference lines it replaces (paths relative to the reference repo).  INTEGRATION.md
 * shows the binding.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. a torch allocation),
 *     fp32, contiguous, 16-byte aligned where noted; the library never allocates or frees
 *     caller-visible memory and never synchronises with the host;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - returns 0 on success or a negative SNR_E_* code; nothing is thrown across the ABI;
 *   - re-entrant and thread-safe: no global mutable state.
 *
 * Layout vocabulary:  N rays, S samples per ray, P = N*S sample points, B objects
 * (object-major: ray r belongs to object r / (N/B), src/model_supnerf.py:246-249),
 * W = 256 hidden width / latent width, NLAT = shape_blocks + texture_blocks latent terms.
 */
#ifndef SUPNERF_HIP_H
#define SUPNERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNR_ABI_VERSION 27

enum {
    SNR_OK = 0,
    SNR_E_ARG = -1,        /* null pointer / bad size / unsupported hyper-parameter */
    SNR_E_SHAPE = -2,      /* sizes inconsistent with each other */
    SNR_E_WORKSPACE = -3,  /* workspace too small */
    SNR_E_LAUNCH = -4,     /* hipLaunchKernel failed (see snr_last_hip_error) */
    SNR_E_UNSUPPORTED = -5
};

/* how per-sample depths are laid out.
 * SNR_Z_BOX: no depth table at all -- the kernel derives every ray's depths itself, the way family B does
 * (NeRFRenderer.prepare_sampled_rays + sample_from_ray, src/renderer.py:27-41,91-115):
 *   o_n = rays_o / z_scale[obj]                           (`rays_o / (obj_diag / 2)`, :103)
 *   slab test of (o_n, rays_d) against the box +-box_half[obj] (ray_box_intersection_tensor, src/utils.py:283-327; NaN-propagating
 *   min / max like torch's), near = far = -1 for rays that miss (:106-108)
 *   u_s = s / S + jitter * (1 / S),  t_s = near (1 - u_s) + far u_s          (:33-41; S a power of two)
 *   p = o_n + t d (xyz_div is NOT applied), composite depth |p - o_n| z_scale with SNR_METRIC_Z (:114)
 * `t_vals` then is the (N,S) jitter in [0,1) (the reference's rand_like draw), or NULL: the kernel draws it itself with
 * Philox4x32-10 (see rng_* below).  The backward kernel returns the gradient THROUGH the bounds to rays_o / rays_d like the
 * reference's autograd (maximum / minimum split ties evenly, as torch does) unless SNR_BOX_DETACH is set.
 * Rules of the slab test and of its gradient (tests/test_special_rays_gpu.py):
 *   1. a NaN in the slab test (0 * inf: rays_d[a] == +-0 with o_n[a] exactly on that face) makes the ray a miss and reaches no output;
 *   2. ties in maximum / minimum split the gradient evenly: 1/2-1/2 through a box edge, 1/4-1/4-1/2 through a corner (two nested maximum);
 *   3. an axis with rays_d[a] == +-0 adds exactly nothing to the gradient of the bounds (0 gradient * infinite 1/d is 0; torch: NaN);
 *   4. the comparisons are strict: t_far > t_near (touching an edge is a miss) and t_far > 0 (a box behind the origin is a miss); an
 *      origin inside the box is a hit with near < 0. */
enum { SNR_Z_SHARED = 0 /* (S,) */, SNR_Z_PER_OBJECT = 1 /* (B,S) */, SNR_Z_PER_RAY = 2 /* (N,S) */, SNR_Z_BOX = 3 /* none: box bounds */ };

/* arithmetic of the decoder GEMMs.  SNR_FP32: v_mfma_f32_32x32x2_f32, bit-for-bit an fp32 fmaf chain.
 * SNR_BF16X3: every fp32 operand split into two 16-bit pieces hi + lo, three 16-bit MFMAs per product, fp32 accumulate (5x less
 * matrix time).  The FORWARD launches carry fp16 pieces (22 bits per operand, relative error ~2^-22 per product; activations are
 * clamped to +-65504, weights likewise at packing time), the BACKWARD launches and snr_weight_grad bf16 pieces (~2^-17: gradients need
 * the exponent range).  Needs shape_blocks + texture_blocks <= 4 and whole 32-point tiles per object;
 * snr_precision_supported() tells. */
enum { SNR_FP32 = 0, SNR_BF16X3 = 1 };
int snr_precision_supported(int precision, int shape_blocks, int texture_blocks, int64_t points_per_obj);

/* flags for the render / composite entry points */
enum {
    SNR_WHITE_BKGD = 1,    /* rgb += 1 - sum(w)            (src/renderer.py:60-63,374-377) */
    SNR_METRIC_Z   = 2,    /* composite depth = |t*d|*z_scale (src/renderer.py:114) instead of t */
    SNR_BOX_DETACH = 4     /* SNR_Z_BOX: the bounds carry no gradient (render_rays_v3 runs its slab test in numpy, src/renderer.py:425-432) */
};

int snr_abi_version(void);
/* text of the last HIP runtime error seen by this thread (for SNR_E_LAUNCH) */
const char* snr_last_hip_error(void);

/* ------------------------------------------------------------------------------------
 * Decoder weights.  The decoder is src/model_supnerf.py:184-199 (== model_codenerf.py:22-37):
 * width 256, latent 256, num_xyz_freq 10, num_dir_freq 4 (every shipped config).
 * `tensors` is a HOST array of 2*(shape_blocks+texture_blocks+6) DEVICE pointers holding the
 * per-point layers in this order, weight then bias, nn.Linear layout (out,in):
 *   encoding_xyz.0, shape_layer_1.0 .. shape_layer_SB.0, encoding_shape, sigma.0,
 *   encoding_viewdir.0, texture_layer_1.0 .. texture_layer_TB.0, rgb.0, rgb.2
 * (the *_latent_layer_* tensors are per-object work and stay with the caller).
 * The packed buffer holds the k-chunked forward stream, the transposed stream for the
 * backward pass and the small vectors; its size in bytes is snr_packed_bytes().
 * ---------------------------------------------------------------------------------- */
size_t snr_packed_bytes(int shape_blocks, int texture_blocks);
int snr_pack_weights(const float* const* tensors, int n_tensors, int shape_blocks, int texture_blocks,
                     float* packed, void* stream);

/* ------------------------------------------------------------------------------------
 * Decoder on explicit sample points: replaces SUPNeRF.forward / CodeNeRF.forward
 * (src/model_supnerf.py:241-269, src/model_codenerf.py:39-63).
 *   xyz, viewdir : (P,3)   object-frame points and unit directions
 *   latent       : (B,NLAT,256) z_j = ReLU(Lin_j(code)), the terms added before each block
 *   points_per_obj = P / B
 *   sigmas (P), rgbs (P,3) outputs (softplus density, raw linear colour)
 *   relu_masks   : NULL, or snr_mask_bytes(P,...) bytes that the backward pass needs
 *   activations  : NULL, or (shape_blocks+texture_blocks+4, P, 256) floats: training mode, receives the INPUT of every
 *                  MFMA layer after the first (slot l = input of layer l+1; the last slot = input of rgb.2, 128 columns
 *                  used).  Needs relu_masks; both precisions.  Together with `layer_grads` of snr_decoder_bwd and the encodings of
 *                  snr_pe_points they are the X operands of the weight-gradient products dW_l = G_l^T X_l of snr_weight_grad (the weight
 *                  half of the backward of src/trainer_unified_nuscenes.py:334).
 * Input range (measured on the MI355X, tests/test_decoder_range_gpu.py; both precisions, every kernel of this section and the
 * density-only ones):
 *   1. Coordinates of any finite size are encoded to fp32 accuracy: angles 2^f x up to 8192 by the kernels' own sin / cos (9.2e-8 of
 *      float64), beyond by the library routine.  SNR_BF16X3 additionally clamps activations to +-65504 (they saturate, finite) and
 *      carries what is smaller than 2^-3 with an absolute 2^-24 instead of 22 relative bits: fp16 subnormal pieces are kept, and a
 *      decoder whose activations or weights are 2^-16 of the usual scale comes out 5e-5 .. 1.3e-4 off (finite).
 *   2. A NaN or an infinity in xyz, viewdir or latent is NOT propagated the way torch.relu propagates it.  The ReLU is a v_med3 (fmaxf in
 *      the fused exact-fp32 forward), which returns the smaller of the other two operands for a NaN: every NaN pre-activation becomes 0 at
 *      the first ReLU behind the poison, and the point returns FINITE values -- those of the decoder with that layer's output forced to
 *      0: encoding_xyz's for a coordinate (sigmas and rgbs both wrong), encoding_viewdir's for a direction (sigmas exact, rgbs wrong), the
 *      next shape / texture layer's for a latent term (every point of that object).  The reference returns NaN there.  Both precisions
 *      return the same values, so comparing them does not reveal the poison: callers that may hold diverged poses or codes check their
 *      inputs themselves.
 *   3. Whatever a poisoned point returns, it changes nothing else: the outputs, ReLU bits, activations and gradients of every other
 *      point, and the d_latent rows of every other object, are bit-identical to those of the clean launch; no call fails.
 * ---------------------------------------------------------------------------------- */
size_t snr_mask_bytes(int64_t n_points, int shape_blocks, int texture_blocks);
int snr_decoder_fwd(const float* xyz, const float* viewdir, const float* latent, const float* packed,
                    int64_t n_points, int64_t points_per_obj, int shape_blocks, int texture_blocks,
                    float* sigmas, float* rgbs, void* relu_masks, float* activations, int precision, void* stream);
/* gradients wrt latent (B,NLAT,256), xyz (P,3), viewdir (P,3) [each nullable] given d_sigmas (P) and d_rgbs (P,3) [each nullable = zero].
 * layer_grads: NULL, or (shape_blocks+texture_blocks+4, P, 256) floats receiving the gradient wrt the pre-activation of
 * every MFMA layer (slot l = layer l; rgb.0 uses 128 columns), both precisions.  workspace: snr_decoder_bwd_ws_bytes(). */
size_t snr_decoder_bwd_ws_bytes(int64_t n_points, int64_t points_per_obj, int shape_blocks, int texture_blocks);
int snr_decoder_bwd(const float* xyz, const float* viewdir, const float* latent, const float* packed,
                    const void* relu_masks, const float* sigmas, const float* d_sigmas, const float* d_rgbs,
                    int64_t n_points, int64_t points_per_obj, int shape_blocks, int texture_blocks,
                    float* d_latent, float* d_xyz, float* d_viewdir, float* layer_grads,
                    void* workspace, size_t ws_bytes, int precision, void* stream);

/* ------------------------------------------------------------------------------------
 * Fused render: sample points on rays -> frame transform -> PE -> decoder -> composite.
 * Replaces the body of render_rays_v2 / render_rays_specified / render_rays /
 * render_full_img after ray generation (src/utils.py:468-500, 523-549, 400-431, 566-600) and
 * of NeRFRenderer.render_rays / render_rays_v3 after the box test
 * (src/renderer.py:108-114,155-166,433-468).
 *   rays_o, rays_d : (N,3) origin and unit direction in the sampling frame
 *   t_vals         : depths along the ray, layout z_mode
 *   xyz_div        : (B,) points are DIVIDED by this (family A: obj_diag, src/utils.py:472)
 *   xyz_mul        : scalar multiplier applied next (render_rays_v3 adjust_scale, src/renderer.py:441)
 *   frame          : 9 floats, row-major 3x3 applied to points and directions afterwards
 *                    (sym flip, kitti2nusc, shapenet_obj_cood: src/utils.py:475-495)
 *   z_scale        : (B,) metric scale for SNR_METRIC_Z (family B: obj_diag/2), else unused
 *   rgb (N,3), depth (N), acc_trans (N) outputs; sigmas (P) / rgbs (P,3) optional per-point outputs
 * Input range: as for the decoder on points (above).  A NaN in a ray's origin reaches every sample of that ray and is erased at
 * encoding_xyz's ReLU: the ray renders FINITE rgb, depth and acc_trans -- those of a ray whose samples all decode with that layer's
 * output 0 -- where the reference returns NaN; every other ray of the launch is bit-identical to the clean launch (measured, SNR_Z_SHARED,
 * both precisions).
 * ---------------------------------------------------------------------------------- */
typedef struct snr_render_args {
    const float* rays_o;
    const float* rays_d;
    const float* t_vals;
    const float* xyz_div;
    const float* z_scale;
    const float* latent;
    const float* packed;
    float frame[9];
    float xyz_mul;
    int32_t z_mode;
    int32_t flags;
    int64_t n_rays;
    int64_t rays_per_obj;
    int32_t n_samples;
    int32_t shape_blocks;
    int32_t texture_blocks;
    int32_t precision;      /* SNR_FP32 / SNR_BF16X3 */
    /* optional (may be null), forward only, (B, NLAT, 256): for every latent term z_j the bias the NEXT layer's accumulators start
     * from, b + W z_j (z_j is added after a ReLU, so it only ever reaches that layer through W z_j; the reference computes
     * `shape_layer_j(y + z_j)`, src/model_supnerf.py:253-263).  With it the split-bf16 forward drops the latent add and its vector
     * loads from every epilogue (-4 %); `latent` is still what the gradient d_latent of snr_render_bwd refers to. */
    const float* latent_bias;
    /* SNR_Z_BOX only: (B,3) half extents of every object's box in the o_n frame, (l, w, h) / diag (src/renderer.py:96-99) */
    const float* box_half;
    /* SNR_Z_BOX with t_vals == NULL: jitter of point i = ray * S + s is the uniform that torch.rand_like of an (N,S) tensor would
     * hold at i for the device generator state (rng_seed, rng_offset) when its kernel runs rng_threads threads (Philox4x32-10:
     * key = seed, counter = (offset / 4 + i / (4 rng_threads), subsequence i % rng_threads), word (i / rng_threads) % 4, value
     * (w + 1) 2^-32 folded to [0,1)).  rng_threads == 0: counter = (offset / 4, subsequence i), word 0. */
    uint64_t rng_seed;
    uint64_t rng_offset;
    uint64_t rng_threads;
} snr_render_args;

int snr_render_fwd(const snr_render_args* a, float* rgb, float* depth, float* acc_trans,
                   float* sigmas, float* rgbs, void* relu_masks, void* stream);
/* backward of the above: upstream d_rgb (N,3), d_depth (N), d_acc (N) [each nullable = zero]
 * -> d_latent (B,NLAT,256), d_rays_o (N,3), d_rays_d (N,3), d_t (layout of t_vals, SNR_Z_PER_RAY only)
 * [each nullable].  Needs sigmas/rgbs/relu_masks saved by the forward. */
size_t snr_render_bwd_ws_bytes(const snr_render_args* a);
int snr_render_bwd(const snr_render_args* a, const float* sigmas, const float* rgbs, const void* relu_masks,
                   const float* d_rgb, const float* d_depth, const float* d_acc,
                   float* d_latent, float* d_rays_o, float* d_rays_d, float* d_t,
                   void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Multi-object scene pixels: replaces the per-pixel depth sort + scatter + volume_rendering3(white) of
 * OptimizerDemo.vis_scene (scripts/demo.py:555-565).  Every pixel carries n_per_pixel = Nb * S samples (the S samples of each of Nb
 * objects; depth -1 marks empty space and carries sigma 0); they are merged by depth and composited.  Samples of exactly equal depth
 * collapse like the reference's scatter: the last one in memory order survives.
 * run_length: S when each object's S samples are contiguous and ascending in depth (what vis_scene produces: stratified samples along
 * the object's ray, or all -1) -- the lists are then MERGED (binary searches, O(n log S Nb) per pixel) instead of rank-sorted (O(n^2));
 * the order is verified per pixel and a pixel with an unsorted list silently takes the rank sort, so the hint can never change a result.
 * 0 = no such structure.  Lists of 32, 64 or 128 samples with n_per_pixel <= 256 take two launches on the stream: a fast pass for pixels
 * without equal depths inside or across increasing lists (it marks the others in `rgb`) and the general kernel for the marked pixels.
 * sigmas, z_vals (P, n); rgbs (P, n, 3) -> rgb (P,3), depth (P) [nullable], acc_trans (P) [nullable].
 * flags: SNR_WHITE_BKGD.  n_per_pixel <= 1706 (LDS).
 * ---------------------------------------------------------------------------------- */
int snr_scene_composite_fwd(const float* sigmas, const float* rgbs, const float* z_vals, int64_t n_pixels, int n_per_pixel, int run_length,
                            int flags, float* rgb, float* depth, float* acc_trans, void* stream);
/* Backward of the above.  Per pixel, with n = n_per_pixel samples i = 0..n-1 in memory order:
 *   lt_i = #{j : z_j < z_i},  eb_i = #{j < i : z_j == z_i},  ea_i = #{j > i : z_j == z_i};
 *   sample i owns slot pos_i = lt_i + eb_i (a permutation) and the sorted depth row is zs[pos_i] = z_i;
 *   slot lt_i receives (sigma_i, rgb_i) from its group's survivor, the member with ea_i == 0 (the last in memory order); the group's
 *   other slots hold sigma 0 and rgb 0;
 *   the sorted rows are composited like every ray here: relu on sigma, last interval 1e10, transmittance + 1e-10, white background.
 * Given d_rgb (P,3), d_depth (P) and d_acc (P) [the last two nullable = zero]:
 *   1. the analytic composite backward runs on the sorted rows and gives every slot (d_sigma, d_r, d_g, d_b, d_z);
 *   2. sample i receives the d_sigma and d_rgb of slot lt_i if it is its group's survivor, and exact zeros otherwise;
 *   3. sample i receives the d_z of its own slot pos_i;
 *   4. at an exact tie the survivor's interval has width 0, so its weight and its sigma gradient are 0 by the formulas: only d_z tells
 *      tied members apart, and rule 3 fixes it;
 *   5. every output element is written exactly once by one lane, without atomics: the same bits from run to run;
 *   6. run_length only changes how the ranks are found (verified per pixel as in the forward): the same bits for 0 and S.
 * -> d_sigmas (P,n), d_rgbs (P,n,3), d_z (P,n) [nullable].  flags: SNR_WHITE_BKGD.  n_per_pixel <= 512 (8 objects x 64 samples), more is
 * SNR_E_UNSUPPORTED.  One launch; tests/scene_grad_restatement.py states the same rules in a few lines of torch. */
int snr_scene_composite_bwd(const float* sigmas, const float* rgbs, const float* z_vals, int64_t n_pixels, int n_per_pixel, int run_length,
                            int flags, const float* d_rgb, const float* d_depth, const float* d_acc,
                            float* d_sigmas, float* d_rgbs, float* d_z, void* stream);

/* ------------------------------------------------------------------------------------
 * Scene rows and samples: what scene.scene_ray_rows and the sample lines of scene.render_scene_batch make with ~65 torch launches, in
 * one launch each way (tests/scene_rows_restatement.py states the same rules in a few lines of torch).
 *   cam2obj (Nb,3,4) camera-in-object poses [R | t] = [R_obj^T | -R_obj^T t_obj];  wlh (Nb,3);  rois (Nb,4) int32 [x0,y0,x1,y1], already
 *   clamped to the image (a pixel outside the image is therefore outside every roi), dead when x1 <= x0 or y1 <= y0;  pixels (Nr,2) int32
 *   (x, y);  jitter (Nr*Nb, S), row r*Nb + b, nullable = 0.  With diag = |wlh|, per pair (pixel r, object b):
 *   coverage   b is live and x0 <= x < x1, y0 <= y < y1;
 *   direction  w = R [(x - cx)/fx, (y - cy)/fy, 1],  u = w / |w|;      origin  o = t / (diag/2);
 *   bounds     rend_aabb: the slab test of (o, u) against +-(l, w, h)/diag -- near = the largest entry, far = the smallest exit; an axis with
 *              u_a == 0 bounds nothing when o_a lies strictly inside its slab and makes the ray a miss otherwise (rules 1, 3, 4 of
 *              SNR_Z_BOX above).  Otherwise the sphere bounds (|t| -/+ diag/2) / (diag/2);
 *   hit        covered and far > near and far > 0 (strict);
 *   depths     z_k = near (1 - tau_k) + far tau_k,  tau_k = k/S + jitter (1/S);
 *   point      (o + z_k u) adjust_scale; shapenet_obj_cood applies (x,y,z) -> (-y,x,z) to the point and to the direction;
 *   metric depth  |z_k u| diag/2.
 * The pair's arithmetic runs in double from the fp32 inputs and every output is rounded to fp32 once.
 * -> xyz, viewdir (Nb*Nr, S, 3) object-major (the decoder's layout), z_vals (Nr, Nb*S) pixel-major (the composite's), hit (Nr,Nb) uint8,
 *    valid (Nr) uint8 [nullable]: some object is hit.  A pair that is not hit holds z_vals = -1 exactly for all S samples, xyz = 0 and
 *    viewdir = (0,0,1): finite inputs for the decoder, whose values there snr_scene_gather_fwd throws away.
 * The lists are only ever compared and converted, never used as an index: the kernels write inside their buffers whatever they hold.
 * Every output element is written once; no host synchronisation; n_pixels == 0 returns at once.  n_objects <= 65535.
 * ---------------------------------------------------------------------------------- */
int snr_scene_samples_fwd(const float* cam2obj, const float* wlh, const int32_t* rois, const int32_t* pixels, float fx, float fy, float cx, float cy,
                          const float* jitter, int64_t n_pixels, int64_t n_objects, int n_samples, float adjust_scale, int rend_aabb,
                          int shapenet_obj_cood, float* xyz, float* viewdir, float* z_vals, uint8_t* hit, uint8_t* valid, void* stream);
/* Backward of the above to the poses: d_xyz, d_viewdir (Nb*Nr,S,3), d_z (Nr,Nb*S), each nullable = zero -> d_cam2obj (Nb,3,4) = [dL/dR | dL/dt].
 *   1. pairs that are not hit contribute exact zeros; the roi is a constant; jitter, pixels and wlh are data;
 *   2. near and far carry the gradient of the one slab plane that gives them, (plane - o_a)/u_a: an axis with u_a == 0 never bounds a hit
 *      and adds nothing (no 0 * inf).  Which plane takes it when two axes give exactly the same parameter is unspecified;
 *   3. the metric depth's gradient to u lies along u and vanishes in u = w/|w|; to z_k it is sign(z_k) diag/2;
 *   4. the same bits from run to run: per-sample arithmetic and all sums in double, no floating-point atomics -- every thread adds its samples
 *      in index order, a workgroup adds its threads' sums in thread order (LDS), and a second launch adds the per-slice rows (256 pixels of
 *      one object each) in slice order.
 * ws: snr_scene_samples_bwd_ws_bytes(n_pixels, n_objects) bytes, 8-byte aligned.  Two launches on the stream. */
size_t snr_scene_samples_bwd_ws_bytes(int64_t n_pixels, int64_t n_objects);
int snr_scene_samples_bwd(const float* cam2obj, const float* wlh, const int32_t* rois, const int32_t* pixels, float fx, float fy, float cx, float cy,
                          const float* jitter, int64_t n_pixels, int64_t n_objects, int n_samples, float adjust_scale, int rend_aabb,
                          int shapenet_obj_cood, const float* d_xyz, const float* d_viewdir, const float* d_z, float* d_cam2obj, void* ws,
                          size_t ws_bytes, void* stream);
/* The decoder's object-major outputs as the composite's pixel-major rows: sigmas (Nb*Nr*S), rgbs (Nb*Nr*S,3), hit (Nr,Nb) from
 * snr_scene_samples_fwd -> sigma_rows (Nr, Nb*S), rgb_rows (Nr, Nb*S, 3); a pair that is not hit holds sigma 0 and white (1,1,1).  Pure
 * copies: the two permutes and two torch.where of scene.render_scene_batch bit for bit.  Either output (with its input) may be NULL. */
int snr_scene_gather_fwd(const float* sigmas, const float* rgbs, const uint8_t* hit, int64_t n_pixels, int64_t n_objects, int n_samples,
                         float* sigma_rows, float* rgb_rows, void* stream);
/* The inverse scatter: d_sigma_rows (Nr, Nb*S), d_rgb_rows (Nr, Nb*S, 3) -> d_sigmas (Nb*Nr*S), d_rgbs (Nb*Nr*S,3), exact zeros on pairs
 * that are not hit.  Either pair may be NULL. */
int snr_scene_gather_bwd(const float* d_sigma_rows, const float* d_rgb_rows, const uint8_t* hit, int64_t n_pixels, int64_t n_objects, int n_samples,
                         float* d_sigmas, float* d_rgbs, void* stream);

/* ------------------------------------------------------------------------------------
 * Scene rows, compact: the same chain with only the (pixel, object) pairs that hit handed to the decoder, `capacity` = C slots per object
 * (tests/scene_compact_restatement.py states the same rules in a few lines of torch).  C >= 1 and C % 32 == 0, so that C * S points are
 * whole 32-point decoder tiles for every S; any other capacity returns SNR_E_ARG before a launch.
 *   hit        per pair exactly what snr_scene_samples_fwd decides (the same code, the same bits): snr_scene_pair_hits writes the flags alone;
 *   scan       hit_scan (Nr,Nb) int32, the CALLER's inclusive prefix sum of hit along the pixel list, per object;
 *   slot       scan[r][b] - 1: the rank of the pair among its object's hits in list order (deterministic, no atomics);
 *   kept       hit and 0 <= slot < C.  A hit pair with slot >= C is DROPPED: every output treats it as a pair that is not hit;
 *   count[b]   scan[Nr-1][b] still tells the true number of hits: max(0, count - C) pairs of object b were dropped;
 *   samples    a kept pair's S points and directions are the bits snr_scene_samples_fwd writes for that pair, at row b*C + slot of xyz and
 *              viewdir (Nb*C, S, 3);  z_vals (Nr, Nb*S) stays pixel-major and dense and holds -1 exactly, for all S samples, on every pair
 *              that is not kept;
 *   padding    slots count[b] .. C-1 of an object: xyz = 0, viewdir = (0,0,1);
 *   pair_of_slot (Nb,C) int32: the pixel index of each slot, -1 on padding;
 *   gather     forward: a kept pair's rows come from its slot, every other pair gets sigma 0 and white.  Backward: written in the
 *              destination's order through pair_of_slot, padding slots get exact zeros;
 *   backward to cam2obj: every kept pair's samples added in the order snr_scene_samples_bwd adds them (the same slice grid, the same
 *              sweep e = thread + i*256, the same LDS meeting order, the same second launch), d_xyz and d_viewdir read at the slot, d_z at
 *              the pair: the same bits as the dense backward of the scattered upstream.  The upstream of padding slots is never read.
 * scan, kept and pair_of_slot are only compared and range-checked, never trusted as an index: the kernels write inside their buffers
 * whatever the lists hold.  Every output element is written once; no host synchronisation and no floating-point atomic; the same bits
 * from run to run.
 * ---------------------------------------------------------------------------------- */
int snr_scene_pair_hits(const float* cam2obj, const float* wlh, const int32_t* rois, const int32_t* pixels, float fx, float fy, float cx, float cy,
                        int64_t n_pixels, int64_t n_objects, int rend_aabb, uint8_t* hit, void* stream);
/* -> xyz, viewdir (Nb*C, S, 3), z_vals (Nr, Nb*S), kept (Nr,Nb) uint8, pair_of_slot (Nb,C) int32.  n_pixels == 0: padding only. */
int snr_scene_samples_compact_fwd(const float* cam2obj, const float* wlh, const int32_t* rois, const int32_t* pixels, float fx, float fy, float cx,
                                  float cy, const float* jitter, int64_t n_pixels, int64_t n_objects, int n_samples, float adjust_scale,
                                  int rend_aabb, int shapenet_obj_cood, const int32_t* hit_scan, int64_t capacity, float* xyz, float* viewdir,
                                  float* z_vals, uint8_t* kept, int32_t* pair_of_slot, void* stream);
/* d_xyz, d_viewdir (Nb*C, S, 3), d_z (Nr, Nb*S), each nullable = zero -> d_cam2obj (Nb,3,4).  ws: snr_scene_samples_bwd_ws_bytes(n_pixels,
 * n_objects) bytes, 8-byte aligned.  Two launches on the stream. */
int snr_scene_samples_compact_bwd(const float* cam2obj, const float* wlh, const int32_t* rois, const int32_t* pixels, float fx, float fy, float cx,
                                  float cy, const float* jitter, int64_t n_pixels, int64_t n_objects, int n_samples, float adjust_scale,
                                  int rend_aabb, int shapenet_obj_cood, const int32_t* hit_scan, int64_t capacity, const float* d_xyz,
                                  const float* d_viewdir, const float* d_z, float* d_cam2obj, void* ws, size_t ws_bytes, void* stream);
/* sigmas (Nb*C*S), rgbs (Nb*C*S,3) -> sigma_rows (Nr, Nb*S), rgb_rows (Nr, Nb*S, 3).  Either output (with its input) may be NULL. */
int snr_scene_gather_compact_fwd(const float* sigmas, const float* rgbs, const int32_t* hit_scan, const uint8_t* kept, int64_t n_pixels,
                                 int64_t n_objects, int n_samples, int64_t capacity, float* sigma_rows, float* rgb_rows, void* stream);
/* d_sigma_rows (Nr, Nb*S), d_rgb_rows (Nr, Nb*S, 3) -> d_sigmas (Nb*C*S), d_rgbs (Nb*C*S,3).  Either pair may be NULL. */
int snr_scene_gather_compact_bwd(const float* d_sigma_rows, const float* d_rgb_rows, const int32_t* pair_of_slot, int64_t n_pixels, int64_t n_objects,
                                 int n_samples, int64_t capacity, float* d_sigmas, float* d_rgbs, void* stream);

/* ------------------------------------------------------------------------------------
 * Alpha composite alone: replaces volume_rendering2 / volume_rendering_batch
 * (src/utils.py:202-233), NeRFRenderer.volume_render (src/renderer.py:43-65) and
 * volume_rendering3 (src/renderer.py:355-379).
 *   sigmas (N,S), rgbs (N,S,3), z_vals per z_mode (per-object: ray r uses row r / rays_per_obj)
 * ---------------------------------------------------------------------------------- */
int snr_composite_fwd(const float* sigmas, const float* rgbs, const float* z_vals, int z_mode, int flags,
                      int64_t n_rays, int64_t rays_per_obj, int n_samples,
                      float* rgb, float* depth, float* acc_trans, void* stream);
/* d_z (layout of z_vals) is produced only for SNR_Z_PER_RAY; pass NULL otherwise */
int snr_composite_bwd(const float* sigmas, const float* rgbs, const float* z_vals, int z_mode, int flags,
                      int64_t n_rays, int64_t rays_per_obj, int n_samples,
                      const float* d_rgb, const float* d_depth, const float* d_acc,
                      float* d_sigmas, float* d_rgbs, float* d_z, void* stream);

/* ------------------------------------------------------------------------------------
 * Sample encoding alone: ray packet -> sample points (+ optional positional encoding).
 * Replaces sample_from_rays + the in-place frame edits (src/utils.py:154-167,472-495), the
 * point/metric-depth part of NeRFRenderer.prepare_sampled_rays (src/renderer.py:111-114) and
 * PE (src/model_supnerf.py:155-161).  Arguments as snr_render_args; outputs
 *   xyz (N,S,3), viewdir (N,S,3), z_out (N,S) [nullable], pe_xyz (N,S,63) [nullable],
 *   pe_dir (N,27) [nullable; constant along S], hit (N) [nullable; SNR_Z_BOX: 1 where the ray meets its box, the
 *   `intersect` map of prepare_sampled_rays]
 * ---------------------------------------------------------------------------------- */
int snr_encode_fwd(const snr_render_args* a, float* xyz, float* viewdir, float* z_out,
                   float* pe_xyz, float* pe_dir, uint8_t* hit, void* stream);
/* The per-object latent layers of a frozen decoder in one launch (src/model_supnerf.py:253,261; model_codenerf.py:50,58):
 *   z[b][j] = ReLU(code_j[b] W_j^T + b_j), j < shape_blocks reads the shape code, the rest the texture code  -> z (B, n_lat, 256)
 *   latent_bias[b][j] = b_next_j + z[b][j] W_next_j^T   [nullable]: what snr_render_args::latent_bias takes
 * with the weights STACKED and TRANSPOSED once by the host: w_lat (512, n_lat*256) -- rows 0..255 multiply the shape code, rows 256..511
 * the texture code, column block j = layer j, zero where a layer does not read that code -- b_lat (n_lat*256), w_nxt (n_lat*256, n_lat*256)
 * block diagonal (block j = shape_layer_{j+1} / texture_layer_{..}.0.weight^T), b_nxt (n_lat*256).  shapecode, texturecode (B,256).
 * snr_latent_bwd: d_z (B, n_lat, 256) -> d_shapecode, d_texturecode (B,256) [each nullable] through the ReLU (z > 0) and W_j; a code no
 * layer reads gets zeros.  (Weight gradients of the latent layers: not here -- training mode keeps them on torch.) */
int snr_latent_fwd(const float* shapecode, const float* texturecode, const float* w_lat, const float* b_lat, const float* w_nxt, const float* b_nxt,
                   int64_t n_objects, int shape_blocks, int texture_blocks, float* z, float* latent_bias, void* stream);
int snr_latent_bwd(const float* d_z, const float* z, const float* w_lat, int64_t n_objects, int shape_blocks, int texture_blocks,
                   float* d_shapecode, float* d_texturecode, void* stream);
/* Positional encodings of explicit points (PE, src/model_supnerf.py:155-161) in the layout the training step's weight-gradient products
 * read: xyz, viewdir (P,3) -> out (P,96), 16-byte aligned: columns 0..62 = PE(xyz, 10 frequencies), 63 = 0, 64..90 = PE(viewdir, 4
 * frequencies), 91..95 = 0 -- the input of encoding_xyz and the direction features of encoding_viewdir (X of their dW = G^T X). */
int snr_pe_points(const float* xyz, const float* viewdir, int64_t n_points, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * Loss / metric tail of one optimise iteration: replaces the three masked reductions the callers run right after the render
 * (src/optimizer_nuscenes.py:729-744 == src/optimizer_kitti.py:792-812; per object of a batch:
 * src/trainer_unified_nuscenes.py:133-140).  Rays are object-major, rays_per_obj per object, B = n_rays / rays_per_obj:
 *   a = |occ|, den = sum(a) + 1e-9
 *   loss_rgb = sum((rgb - rgb_tgt)^2 a) / den        loss_occ = sum(exp(-occ (0.5 - acc_trans)) a) / den
 *   loss     = loss_rgb + loss_occ_coef * loss_occ   mse_fg   = sum((rgb - rgb_tgt)^2 max(occ, 0)) / (sum(max(occ, 0)) + 1e-9)
 * rgb, rgb_tgt (N,3); acc, occ (N) -> out (B,4) = [loss, loss_rgb, loss_occ, mse_fg]  (PSNR = -10 log10 mse_fg, :743).
 * snr_loss_tail_bwd writes the gradient seeds of the render backward, d(sum_b upstream_b loss_b)/d rgb (N,3) and /d acc (N)
 * [each nullable]; upstream (B,) nullable = ones.  One launch each, no host synchronisation.
 * ---------------------------------------------------------------------------------- */
int snr_loss_tail_fwd(const float* rgb, const float* acc, const float* rgb_tgt, const float* occ, int64_t n_rays, int64_t rays_per_obj,
                      float loss_occ_coef, float* out, void* stream);
int snr_loss_tail_bwd(const float* rgb, const float* acc, const float* rgb_tgt, const float* occ, int64_t n_rays, int64_t rays_per_obj,
                      float loss_occ_coef, const float* upstream, float* d_rgb, float* d_acc, void* stream);

/* ------------------------------------------------------------------------------------
 * The rest of one iteration of the test-time optimisation loop (src/optimizer_nuscenes.py:674-783 == src/optimizer_kitti.py:731-866),
 * one launch each, B objects per launch (one workgroup per object), nothing synchronises with the host.
 *
 * snr_pose_rays_fwd: the optimised parameters rot_vec (B,3) [axis-angle; pytorch3d axis_angle_to_matrix in the reference, :666,:686] and
 *   trans_vec (B,3) -> camera-in-object pose cam2opt (B,3,4) [= the inverse of the object pose unless opt_cam_pose, :690-699], then what
 *   render_rays_v2 derives from it: rays_o / unit viewdir (B*n,3) of the object's pixels (get_rays, src/utils.py:107-135; cam_dirs (B,n,3) =
 *   [(px-cx)/fx, (py-cy)/fy, 1] is constant over the loop), near/far = |camera centre| -/+ half_diag (:468-469) and the stratified depth
 *   vector z_vals (B,S) of sample_from_rays (:159-164) with the given jitter (B,S) [nullable = 0].  cam2opt / z_vals nullable.
 * snr_pose_rays_bwd: d_rays_o, d_viewdir (B*n,3), d_cam2opt (B,3,4) [each nullable] -> d_rot_vec, d_trans_vec (B,3).  The depths are
 *   detached from the pose like the reference's .tolist().
 * ---------------------------------------------------------------------------------- */
int snr_pose_rays_fwd(const float* rot_vec, const float* trans_vec, const float* cam_dirs, const float* half_diag, const float* jitter,
                      int64_t n_objects, int64_t rays_per_obj, int n_samples, int opt_cam_pose,
                      float* cam2opt, float* rays_o, float* viewdir, float* z_vals, void* stream);
int snr_pose_rays_bwd(const float* rot_vec, const float* trans_vec, const float* cam_dirs, int64_t n_objects, int64_t rays_per_obj,
                      int opt_cam_pose, const float* d_rays_o, const float* d_viewdir, const float* d_cam2opt,
                      float* d_rot_vec, float* d_trans_vec, void* stream);
/* The same two launches for a caller that holds the camera pose itself -- what the public get_rays / render_rays_v2 do per call
 * (src/utils.py:107-135 get_rays, :468-469 sphere bounds, :159-164 sample_from_rays' depth vector): c2w (B,3,4) row-major [R | t]
 * -> rays_o / unit viewdir (B*n,3) and the stratified depths z_vals (B,S) [z_vals, half_diag, jitter nullable]; backward:
 * d_rays_o, d_viewdir (B*n,3) [each nullable] -> d_c2w (B,3,4).  The depths are detached from the pose like the reference's. */
int snr_cam_rays_fwd(const float* c2w, const float* cam_dirs, const float* half_diag, const float* jitter, int64_t n_objects,
                     int64_t rays_per_obj, int n_samples, float* rays_o, float* viewdir, float* z_vals, void* stream);
int snr_cam_rays_bwd(const float* c2w, const float* cam_dirs, int64_t n_objects, int64_t rays_per_obj, const float* d_rays_o,
                     const float* d_viewdir, float* d_c2w, void* stream);
/* The metric row the loop logs every iteration (:739-765): row (B,4) = [PSNR = -10 log10(loss_out[:,3]), depth error, rotation error
 * rot_dist(pred_R, gt_R) (src/utils.py:713-722), translation error |pred_t - gt_T|]; gt_R (B,3,3), gt_T (B,3) are the true OBJECT pose,
 * cam2opt the current camera-in-object pose.  Depth error of object b = sum_i |depth_pred[b,i] - depth0[b,i]| / (count_b + 1e-8) over its
 * first count_b = lidar_count[b] (int32, nullable = n_lidar for every object) of the n_lidar columns: with depth0 = the lidar
 * measurements and first = 0 this is log_eval_depth_v2 (src/optimizer_nuscenes.py:751-765,1736-1741); first != 0 stores
 * depth0 <- depth_pred instead (objects without a depth map: the change of rendered depth against the first iteration is logged). */
int snr_metric_row(const float* loss_out, const float* depth_pred, float* depth0, int n_lidar, int first, const float* cam2opt,
                   const float* gt_R, const float* gt_T, int64_t n_objects, int opt_cam_pose, float* row, const int32_t* lidar_count,
                   void* stream);
/* torch.optim.AdamW's update (amsgrad off) of up to 4 parameter groups in one launch (:1762-1769): HOST arrays of n_groups device
 * pointers / element counts / learning rates; step = 1 for the first update. */
int snr_adamw_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numel,
                   const float* lr, int n_groups, int64_t step, float beta1, float beta2, float eps, float weight_decay, void* stream);
/* The same update for any number of tensors in ONE launch: the training step's optimiser (src/trainer_unified_nuscenes.py:414-422, AdamW over
 * every decoder tensor and the two code tables).  table: DEVICE memory, n_tensors entries of six 64-bit words
 * {param*, grad*, exp_avg*, exp_avg_sq*, numel, group} (fp32 contiguous tensors; group < n_groups selects the learning rate lr[group],
 * a HOST array); max_numel = the largest numel in the table; step = 1 for the first update. */
int snr_adamw_table_step(const void* table, int n_tensors, int64_t max_numel, const float* lr, int n_groups, int64_t step, float beta1, float beta2,
                         float eps, float weight_decay, void* stream);

/* ------------------------------------------------------------------------------------
 * Weight gradient of one decoder layer (training mode): the weight half of loss_total.mean().backward()
 * (src/trainer_unified_nuscenes.py:334) for y = x W^T + b (nn.Linear, src/model_supnerf.py:184-199):
 *     dW (n_out, n_in; leading dimension ld_dw) = G^T X,   db (n_out) = column sums of G [nullable]
 * G (P, n_out; leading dimension ldg) = gradient wrt the layer's pre-activation = slot l of snr_decoder_bwd's layer_grads;
 * X (P, n_in; leading dimension ldx) = the layer's input = slot l-1 of snr_decoder_fwd's activations (or the positional encoding).
 * precision SNR_FP32: exact fp32 on the matrix cores; SNR_BF16X3: the split-bf16 products of the render fast path (operand error ~2^-17,
 * 5x less matrix time, HBM-bound); the narrow heads and the bias sums are always fp32.  Split over the points, per-slice partials summed
 * in slice order (deterministic, no atomics).
 * n_out, n_in <= 256.  n_out >= 32: n_out, n_in, ldg, ldx multiples of 4 and G, X 16-byte aligned; n_out <= 4 (density / colour head):
 * no alignment requirement.  workspace: snr_weight_grad_ws_bytes().
 * ---------------------------------------------------------------------------------- */
size_t snr_weight_grad_ws_bytes(int64_t n_points, int n_out, int n_in);
int snr_weight_grad(const float* G, int64_t ldg, int n_out, const float* X, int64_t ldx, int n_in, int64_t n_points,
                    float* dW, int64_t ld_dw, float* db, int precision, void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Geometry: the density of a shape code on a lattice, and the iso-surface of such a grid.
 *
 * A lattice (HOST struct, like snr_render_args) is n[0] x n[1] x n[2] points, 1 <= n[a] <= 512, point (i0, i1, i2) at
 * lo[a] + h[a] * i_a per axis, evaluated as one fp32 multiply and one fp32 add (no fma).  A grid of B objects is (B, n0, n1, n2) floats,
 * object-major, then axis 0 (x) major, axis 2 (z) fastest: linear index v = (i0 n1 + i1) n2 + i2.
 * ---------------------------------------------------------------------------------- */
typedef struct snr_lattice {
    float lo[3];
    float h[3];
    int32_t n[3];
} snr_lattice;

/* Density-only decoder, exact fp32: the chain of snr_decoder_fwd with SNR_FP32 up to the density head and nothing after it (no view
 * direction, no encoding_viewdir, texture or rgb layers).  sigmas is bit-identical to the sigmas snr_decoder_fwd returns for the same
 * points, packed weights (texture rows present, unread) and latent terms (B,NLAT,256).
 * snr_density_fwd: xyz (P,3), points_per_obj = P / B, sigmas (P).
 * snr_density_grid: the points of `lattice` for each of n_objects objects, generated in the kernel; sigmas (B, n0, n1, n2). */
int snr_density_fwd(const float* xyz, const float* latent, const float* packed, int64_t n_points, int64_t points_per_obj,
                    int shape_blocks, int texture_blocks, float* sigmas, void* stream);
int snr_density_grid(const snr_lattice* lattice, int64_t n_objects, const float* latent, const float* packed, int shape_blocks,
                     int texture_blocks, float* sigmas, void* stream);
/* snr_density_fwd plus the ReLU bits of encoding_xyz and the shape layers, in snr_decoder_fwd's relu_masks layout
 * (snr_mask_bytes(P, sb, tb) bytes; texture-branch slots are not written). sigmas bit-identical to snr_density_fwd. */
int snr_density_fwd_masks(const float* xyz, const float* latent, const float* packed, int64_t n_points, int64_t points_per_obj,
                          int shape_blocks, int texture_blocks, float* sigmas, void* relu_masks, void* stream);
/* Backward of snr_density_fwd: d_xyz (P,3) and d_latent (B,NLAT,256; texture rows zero), each nullable, given d_sigmas (P).
 * d_latent needs points_per_obj % 64 == 0 (else SNR_E_UNSUPPORTED); workspace: snr_decoder_bwd_ws_bytes().
 * relu_masks, sigmas: from snr_density_fwd_masks (or snr_decoder_fwd) on the same points.  d_xyz and the shape rows of d_latent are
 * bit for bit those of snr_decoder_bwd with SNR_FP32 and d_rgbs = 0 (zeros of either sign compare equal). */
int snr_density_bwd(const float* xyz, const float* latent, const float* packed, const void* relu_masks, const float* sigmas,
                    const float* d_sigmas, int64_t n_points, int64_t points_per_obj, int shape_blocks, int texture_blocks,
                    float* d_latent, float* d_xyz, void* workspace, size_t ws_bytes, void* stream);

/* Iso-surface of n_grids grids on `lattice` (2 <= n[a] <= 512) by marching tetrahedra on the Kuhn split.  A sample is inside iff
 * value > level.  Cell (i0, i1, i2) (index c = (i0 (n1-1) + i1) (n2-1) + i2) has corners v000 + bits (bit a = +1 on axis a) and splits
 * into 6 tetrahedra v000 -> v000+e_a -> v000+e_a+e_b -> v111, one per permutation (a,b,c) in the order 012, 021, 102, 120, 201, 210.
 * Every tetrahedron edge is a grid edge from its lower endpoint u in one of 7 directions d (0..6 = x, y, z, xy, xz, yz, xyz), edge id
 * 7 u + d.  One vertex per crossing edge, in edge-id order: t = (level - f(u)) / (f(u+d) - f(u)), coordinate lo + h (i + t d) per axis,
 * every step rounded to fp32.  Faces (int32 vertex indices, local to the object) in the order cell, tetrahedron, triangle: one triangle
 * for 1 or 3 corners inside, two for 2 (the quad split along the diagonal through its vertex of smallest edge id), counter-clockwise
 * seen from the outside (the low side); tests/iso_restatement.py states the whole rule set step by step.
 *
 * Pass 1, snr_iso_count: tri_count (B, cells) uint8 triangles per cell, edge_mask (B, n0 n1 n2) uint8 crossing edges per grid vertex
 * (bit d), edge_count (B, n0 n1 n2) uint8 = popcount(edge_mask).
 * The caller then scans per object: tri_scan, edge_scan = the INCLUSIVE int32 prefix sums of tri_count and edge_count along each
 * object's row, and vert_offset, tri_offset (B) int64 = where each object's vertices / triangles start in the output.
 * Pass 2, snr_iso_emit: verts (sum V, 3) fp32, faces (sum F, 3) int32. */
int snr_iso_count(const float* grid, int64_t n_grids, const snr_lattice* lattice, float level, uint8_t* tri_count, uint8_t* edge_mask,
                  uint8_t* edge_count, void* stream);
int snr_iso_emit(const float* grid, int64_t n_grids, const snr_lattice* lattice, float level, const uint8_t* edge_mask,
                 const int32_t* edge_scan, const int32_t* tri_scan, const int64_t* vert_offset, const int64_t* tri_offset, float* verts,
                 int32_t* faces, void* stream);

/* Narrow band: the density of a lattice (2 <= n[a] <= 512) evaluated only in the bricks the surface {value = level} crosses.
 * Brick (I, J, K) owns the points [8I, 8I+8) x [8J, 8J+8) x [8K, 8K+8) inside the grid; nb[a] = ceil(n[a] / 8) bricks per axis, brick
 * index r = (I nb1 + J) nb2 + K.  The coarse lattice is the lattice's points at multiples of 8, one more per axis past the far edge: lo,
 * h' = 8 h (exact in fp32), nb[a] + 1 points; since 8 h I and h 8 I are the same real product, snr_density_grid on it gives bit for bit
 * the values of the fine lattice at every coarse point inside the grid.  Its (B, nb0+1, nb1+1, nb2+1) grid gives each brick 8 corners.
 *
 * snr_density_bricks: the density forward (bit-identical to snr_density_grid) at the 512 points of each brick of the list `bricks`
 * (n_bricks, 4) int32 = (object, I, J, K), stored into sigmas (B, n0, n1, n2) at the points inside the grid; no other value is written.
 * A brick whose object or coordinates are out of range is skipped.
 * snr_band_classify: per brick of the coarse grid `coarse`: state (B, nb0 nb1 nb2) int32 = 1 (active) when its 8 corners are not all
 * on one side of the level (inside iff value > level), when a corner c has |c - level| <= band (fp32), or when a corner is not finite;
 * else 0.  fill (same shape) float = the largest corner when all 8 are inside, else the smallest (a one-sided brick: the corner farthest
 * from the level); NaN when a corner is not finite.
 * snr_band_compact: every brick with state 1 into bricks (object, I, J, K) at row scan[r] - 1, scan = the INCLUSIVE int32 prefix sum of
 * (state == 1) over the whole (B, nb0 nb1 nb2) array: object-major, brick order within an object.
 * snr_band_fill: every grid point of a brick with state 0 takes the brick's fill value; other points are not written.
 * snr_band_seam (stamp >= 2): a brick counts as evaluated iff 1 <= state < stamp.  Every grid edge of the iso rules' 7 directions whose
 * endpoints are on different sides of the level and not both evaluated moves the bricks of its unevaluated endpoints from state 0 to
 * stamp, each brick once, appends them to bricks (object, I, J, K) (in no fixed order) and counts them in *n_new (device int32, set to 0
 * first).  The set of bricks does not depend on the order of the threads.  At the fixpoint (n_new = 0 after the bricks of every state have
 * been evaluated) every crossing edge of the grid has both endpoints exact, and the iso-surface of the grid equals that of the dense grid
 * wherever the coarse pass found the surface; tests/band_restatement.py restates the whole loop. */
int snr_density_bricks(const snr_lattice* lattice, int64_t n_objects, const int32_t* bricks, int64_t n_bricks, const float* latent,
                       const float* packed, int shape_blocks, int texture_blocks, float* sigmas, void* stream);
int snr_band_classify(const float* coarse, int64_t n_grids, const snr_lattice* lattice, float level, float band, int32_t* state, float* fill,
                      void* stream);
int snr_band_compact(const int32_t* state, const int32_t* scan, int64_t n_grids, const snr_lattice* lattice, int32_t* bricks, void* stream);
int snr_band_fill(float* grid, int64_t n_grids, const snr_lattice* lattice, const int32_t* state, const float* fill, void* stream);
int snr_band_seam(const float* grid, int64_t n_grids, const snr_lattice* lattice, float level, int32_t stamp, int32_t* state, int32_t* bricks,
                  int32_t* n_new, void* stream);

/* Iso-surface backward: vertex gradients of snr_iso_emit's output to the grid values, and the grid points the surface touches.
 * The derivative is the one of the piecewise function whose topology (edge_mask) is the forward's: topology changes carry no gradient,
 * and the level gets none.  A vertex on crossing edge (u, d) has va = f(u), vb = f(u + d) (one of them > level, the other not), so
 * t = (level - va) / (vb - va) and c_a = lo_a + h_a (i_a + t d_a).  For its upstream gradient g (3 floats):
 *   s = sum over the axes a with d_a = 1 of g_a h_a, in axis order, fp32 (s = 0 + g_a h_a + ...);
 *   w = s / ((vb - va) * (vb - va));
 *   d f(u) += w * (level - vb),  d f(u + d) += w * (va - level).
 * vb - va is never zero on a crossing edge but can be tiny: the gradient is then large.  That is inherent to an iso-surface at fixed
 * topology; nothing is clamped.
 *
 * snr_iso_grad: d_verts (sum V, 3) fp32, laid out as snr_iso_emit wrote verts (vert_offset, edge_mask, edge_scan of the same forward) ->
 * d_grid (B, n0, n1, n2) fp32, dense.  Each grid point GATHERS its terms, accumulating acc = 0 + term + ... in fp32 in a fixed order:
 * first its outgoing crossing edges d = 0..6 (bit d of its own edge_mask; vertex edge_scan - popc(m) + popc(m & (2^d - 1))), then its
 * incoming ones d = 0..6 (bit d of the point u - dir(d), where that point exists).  No atomics: the result is deterministic.  A point
 * on no crossing edge gets +0.  on_surface (B, n0, n1, n2) uint8 (nullable) = 1 iff the point is an end of at least one crossing edge.
 * snr_iso_surface_points: the flagged points of each object, in grid order, into a list of points_per_obj slots per object (object b at
 * rows b points_per_obj ...): xyz (B points_per_obj, 3) the lattice coordinate lo + h i (one fp32 multiply, one add: snr_density_fwd
 * there returns the value snr_density_grid stored, bit for bit), d_sigmas (B points_per_obj) the point's d_grid.  Slot = scan - 1 with
 * scan the INCLUSIVE int32 prefix sum of on_surface along each object's row; slots from the object's count to points_per_obj are
 * padding: xyz = lo, d_sigmas = 0.  A point whose slot is >= points_per_obj is not written. */
int snr_iso_grad(const float* grid, int64_t n_grids, const snr_lattice* lattice, float level, const uint8_t* edge_mask,
                 const int32_t* edge_scan, const int64_t* vert_offset, const float* d_verts, float* d_grid, uint8_t* on_surface,
                 void* stream);
int snr_iso_surface_points(const uint8_t* on_surface, const int32_t* surface_scan, const float* d_grid, int64_t n_grids,
                           const snr_lattice* lattice, int64_t points_per_obj, float* xyz, float* d_sigmas, void* stream);

/* Ray-cast surfaces: along each ray, the first point where the density rises through `level`.  The decoder work is snr_density_fwd on
 * the point lists made here (and snr_density_fwd_masks / snr_density_bwd at the hit points, for normals and gradients); these entry points
 * are the per-ray passes around it.  R rays (object-major when several objects share a launch), all arithmetic fp32, one rounding per
 * written operation (no fma); tests/ray_restatement.py restates every rule step by step.
 *   1. March of an interval [ta, tb] with S >= 2 samples: step = (tb - ta) / (S - 1); t_k = ta + step * k for k < S - 1 and t_{S-1} = tb
 *      exactly; point p_k = o + t_k * d per axis (one multiply, one add).
 *   2. A sample is inside iff sigma_k >= level (a NaN is outside, +inf inside).
 *   3. First crossing: the smallest k in [0, S - 2] with sigma_k outside and sigma_{k+1} inside; its bracket is
 *      (ta', tb', va, vb) = (t_k, t_{k+1}, sigma_k, sigma_{k+1}).
 *   4. State, decided by the first march only: 2 = sigma_0 inside (the ray starts inside), else 1 = a crossing exists, else 0 = miss.
 *      A ray of state 0 / 2 leaves the first march with the dummy interval [ta, ta] and va = vb = 0.
 *   5. Refinement: the bracket of every state-1 ray is marched again (any S) and replaced by the first crossing of that march.  Both ends
 *      of the sub-march are the bracket's ends bit for bit (rule 1), so it starts outside and ends inside and always has a crossing; a
 *      state-1 ray whose march shows none (sigma not the decoder's) keeps its bracket.  Rays of state 0 / 2 are not touched.
 *   6. Depth: t = ta + (level - va) / (vb - va) * (tb - ta) on state 1 (vb - va > 0), ta (= near) on state 2, 0 on state 0; width
 *      = tb - ta on state 1, else 0: the depth and the true crossing both lie in the bracket.  Hit point x = o + t * d (every state).
 *   7. Normal (state 1): snr_density_fwd_masks + snr_density_bwd with d_sigmas = 1 at x give g = grad sigma(x); slope = g . d summed in
 *      axis order; normal = -g / |g| (the zero vector where |g| is 0 or not finite, and on states 0 / 2).  No gradient flows through it.
 *   8. Gradient of the depth: the implicit function theorem on sigma(o + t d; code) = level at x -- not the derivative of rule 6's
 *      interpolation, which is wrong by percents inside a bracket of a steep density.  With the upstream gradient d_t and
 *      c = -d_t / slope on state 1, 0 elsewhere: d o = c g, d d = t c g, and the latent gradient is snr_density_bwd with d_sigmas = c on
 *      the ReLU bits saved in rule 7 (objects padded to whole 64-point workgroups).  near, far, level and the topology get none; a
 *      grazing ray (slope -> 0) gives a large one and nothing is clamped.  Rules 7 - 8 need no kernel of their own.
 *
 * snr_ray_march_points: rays_o, rays_d (R,3), ta, tb (R) -> xyz (R n_samples, 3), ray-major (rule 1).
 * snr_ray_first_crossing: sigmas (R, n_samples) of the march of [ta, tb]; first = 1: writes state (R) uint8 and the bracket ta, tb, va, vb
 *   (R) IN PLACE (rules 2 - 4); first = 0: reads state, replaces the bracket of state-1 rays (rule 5).
 * snr_ray_hit_points: depth, width (R), xyz (R,3) (rule 6).
 * n_samples < 2 or a null pointer: SNR_E_ARG; more than 2^31 threads (R n_samples points; 64 R from n_samples = 32 on in the crossing
 * search, which then takes a wave per ray): SNR_E_UNSUPPORTED. */
int snr_ray_march_points(const float* rays_o, const float* rays_d, const float* ta, const float* tb, int64_t n_rays, int n_samples,
                         float* xyz, void* stream);
int snr_ray_first_crossing(const float* sigmas, int64_t n_rays, int n_samples, float level, int first, float* ta, float* tb, float* va,
                           float* vb, uint8_t* state, void* stream);
int snr_ray_hit_points(const float* rays_o, const float* rays_d, const float* ta, const float* tb, const float* va, const float* vb,
                       const uint8_t* state, int64_t n_rays, float level, float* depth, float* width, float* xyz, void* stream);

/* Fixed-order segmented sums: how every float64 sum of the packed-mesh entry points below (snr_mesh_segment_sum, snr_simplify_positions,
 * snr_simplify_attributes) runs.  The terms form a list sorted by segment: seg_start (n_segments + 1) int64, ascending, segment k's terms at
 * [seg_start[k], seg_start[k+1]).  A segment's terms are cut into slabs of 4096, the last one short; slab_offset (n_segments + 1) int64 =
 * the EXCLUSIVE prefix sum of ceil(terms / 4096) per segment, so slab s of segment k holds the terms [seg_start[k] + 4096 j, + 4096), j =
 * s - slab_offset[k], and an empty segment has no slab.  Order of every sum: within a slab, thread t of 256 starts from 0.0 and adds the
 * terms t, t + 256, ... in that order, then a binary tree over the threads (k = 128, 64, ..., 1: t += t + k for t < k); per segment, lane l
 * of 64 starts from 0.0 and adds the segment's slab sums l, l + 64, ... in that order, then a butterfly over the lanes (l += l xor 32, 16,
 * ..., 1).  Several channels are summed side by side, each in this order.  The library is built without fused multiply-adds and nothing
 * is added atomically: the bits are those of the order (tests/segment_sum_restatement.py restates it; tests/test_segment_sum_gpu.py holds
 * the kernels to it), the same from run to run.  The slab sums go through a float64 scratch of n_slabs rows, n_slabs >=
 * snr_segment_slab_bound(n_segments, n_items) = n_segments + n_items / 4096 (0 for a negative argument), else SNR_E_WORKSPACE. */
int64_t snr_segment_slab_bound(int64_t n_segments, int64_t n_items);

/* Mesh components: which vertices and faces of a triangle mesh hang together, and what each piece measures.  The mesh is the packed form
 * snr_iso_emit writes, or any caller's of the same form: verts (sum V, 3) fp32 and faces (sum F, 3) int32 of n_objects objects, object
 * after object, face indices local to their object; vert_offset, face_offset (n_objects + 1) int64 DEVICE arrays, ascending, from 0 to
 * n_verts = sum V and n_faces = sum F: where each object's vertices / faces start (V <= 2^31 - 1 per object).
 * tests/mesh_restatement.py restates every rule step by step.
 *   1. Connectivity: two vertices are connected iff a chain of faces links them through shared vertex INDICES.  Equal positions do not
 *      connect: the coincident vertices of a degenerate triangle stay distinct unless a face joins them.  A vertex no face names is a
 *      component of its own with 0 faces.
 *   2. Component ids are local to the object and fully determined by the mesh: component c is the one whose smallest vertex index is the
 *      c-th smallest among the object's components (vertex 0 is always in component 0).  vert_label (sum V) int32; face_label (sum F)
 *      int32 = the label of the face's first vertex.  The components of all objects are packed object after object too: comp_offset
 *      (n_objects + 1) int64, component c of object b at comp_offset[b] + c.
 *   3. Measures per component: n_verts and n_faces (int64, exact); bbox_lo, bbox_hi (C, 3) fp32, the exact min / max of its vertex
 *      coordinates (finite coordinates; -0 and +0 count as equal); area and volume in float64: with a, b, c the face's vertices widened
 *      to float64 and p0 the component's vertex of smallest index,
 *          area term = |(b - a) x (c - a)| / 2,      volume term = (a - p0) . ((b - p0) x (c - p0)) / 6,
 *      each summed over the component's faces.  The volume is signed: the iso rules wind faces counter-clockwise seen from the low side,
 *      so a closed dense blob is positive and a closed cavity negative.  For a closed component the value does not depend on p0; for one
 *      cut open (by the border of the grid) it is this rule's value and no more.  The sums run in a fixed order ("Fixed-order segmented
 *      sums" above): two runs give the same bits.  No floating-point atomics anywhere.
 *   4. Selection: a subset of components gives a sub-mesh -- the kept vertices in their original order, the kept faces in their original
 *      order, indices renumbered.  (Host policy over the labels; no kernel.)
 *
 * snr_mesh_hook: parent (sum V) int32 := the identity per object, then (a second launch) a lock-free union-find over the faces, one thread
 *   per face, uniting (v0, v1) and (v0, v2): the larger root is hooked under the smaller by compare-and-swap, so at the end the root of a
 *   component is its smallest vertex index.  Inside that launch every read of parent is an agent-scope atomic load and every update an
 *   agent-scope compare-and-swap or atomic min (the L2s of the eight XCDs are not coherent with each other); no thread waits for another.
 *   Every face's three indices are range-checked before use: a face with an index outside [0, V) is skipped and *bad (device int32, zeroed
 *   by the caller) is set to 1.
 * snr_mesh_flatten (a later launch: plain loads): root (sum V) int32 = the root above each vertex, is_root (sum V) uint8 = (root == vertex).
 *   The caller then scans per object: root_scan = the INCLUSIVE int32 prefix sum of is_root along each object's vertices; its last entry
 *   is the object's component count C.
 * snr_mesh_label: vert_label[v] = root_scan[root[v]] - 1 (indices within the object), then face_label (rule 2; -1 on a bad first index).
 * snr_mesh_boxes: comp_verts (sum C) int64, bbox_lo, bbox_hi (sum C, 3) of rule 3, by integer atomic add / min / max on order-preserving
 *   keys of the coordinates (exact in any order).  A vertex whose label is not one of its object's components is not counted.
 * snr_mesh_face_terms: the two float64 terms of rule 3 per face; slot i holds face order[i] (order: (sum F) int64, a permutation of the
 *   packed face indices -- the faces sorted by component -- or NULL = as stored).  p0 = the vertex root[v0].  A face with a bad index
 *   gives 0, 0.  An order entry outside [0, sum F) gives its slot 0, 0 too, and nothing is read with it.
 * snr_mesh_segment_sum: area, volume (sum C) float64 from terms sorted by component: seg_start (sum C + 1) int64, component k's terms at
 *   [seg_start[k], seg_start[k+1]), with slab_offset (sum C + 1) int64, both as "Fixed-order segmented sums" above defines them, which
 *   is also the order of the two sums.  partial: (n_slabs, 2) float64 scratch, n_slabs >= snr_segment_slab_bound(sum C, sum F).
 * A null pointer or a negative size: SNR_E_ARG; more than 2^38 vertices, faces or components in a launch: SNR_E_UNSUPPORTED. */
int snr_mesh_hook(const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, int64_t n_objects, int64_t n_verts,
                  int64_t n_faces, int32_t* parent, int32_t* bad, void* stream);
int snr_mesh_flatten(const int32_t* parent, const int64_t* vert_offset, int64_t n_objects, int64_t n_verts, int32_t* root, uint8_t* is_root,
                     void* stream);
int snr_mesh_label(const int32_t* root, const int32_t* root_scan, const int32_t* faces, const int64_t* vert_offset,
                   const int64_t* face_offset, int64_t n_objects, int64_t n_verts, int64_t n_faces, int32_t* vert_label, int32_t* face_label,
                   void* stream);
int snr_mesh_boxes(const float* verts, const int32_t* vert_label, const int64_t* vert_offset, const int64_t* comp_offset, int64_t n_objects,
                   int64_t n_verts, int64_t n_comps, int64_t* comp_verts, float* bbox_lo, float* bbox_hi, void* stream);
int snr_mesh_face_terms(const float* verts, const int32_t* faces, const int32_t* root, const int64_t* order, const int64_t* vert_offset,
                        const int64_t* face_offset, int64_t n_objects, int64_t n_verts, int64_t n_faces, double* area_terms,
                        double* volume_terms, void* stream);
int snr_mesh_segment_sum(const double* area_terms, const double* volume_terms, const int64_t* seg_start, const int64_t* slab_offset,
                         int64_t n_comps, int64_t n_faces, double* partial, int64_t n_slabs, double* area, double* volume, void* stream);

/* Mesh simplification: quadric vertex clustering (Lindstrom 2000) of a packed mesh -- the form of "Mesh components" above (verts, object-
 * local int32 faces, vert_offset and face_offset DEVICE arrays).  Every object b has a cell edge cell[b] > 0 and an origin origin[b] (3),
 * both fp32 DEVICE arrays ((n_objects) and (n_objects, 3)).  tests/simplify_restatement.py restates every rule step by step.
 *   1. Cell of a vertex: q_a = (int32) floorf((x_a - origin_a) / cell), the subtraction and the division each one correctly rounded fp32
 *      operation.  A coordinate exactly on a cell face belongs to the upper cell; -0 counts as 0.  Two vertices of an object fall into one
 *      cluster iff their (qx, qy, qz) are equal.  Connectivity plays no part: two sheets that pass through one cell merge there.  A
 *      non-finite coordinate or a |q_a| >= 2^20 sets *bad (snr_simplify_keys); a face index outside [0, V) sets *bad (snr_simplify_faces).
 *   2. Numbering: the clusters of an object are numbered in ascending lexicographic (qx, qy, qz) order; new vertex k is cluster k.
 *      vert_map (sum V) int32 = the new local index of every old vertex; members (sum V') int32 = the size of each cluster.  The order
 *      comes from the caller's stable sort of the packed keys ((qx + 2^20) << 42 | (qy + 2^20) << 21 | (qz + 2^20), int64) within each
 *      object, head flags and an inclusive scan; it is fully determined by the mesh.
 *   3. Position, mean placement: m = (sum of the members' coordinates widened to float64) / count, rounded to fp32.
 *   4. Position, quadric placement: with c0 = origin + (q + 1/2) cell in float64, over every (face, corner) pair of the ORIGINAL faces
 *      whose corner vertex lies in the cluster (faces that will degenerate included), with a', b', c' the face's vertices minus c0 in
 *      float64:  n = (b' - a') x (c' - a'),  d = -n . a',  A += n n^T (six unique sums),  v += d n (three sums).
 *      tr = A00 + A11 + A22.  If tr <= (1e-12 cell^2)^2 (a cluster touched only by faces without area): x = m.  Otherwise lambda =
 *      SNR_SIMPLIFY_EPS tr, (A + lambda I) y = lambda (m - c0) - v solved in float64 by a 3x3 Cholesky factorisation (m not rounded),
 *      x = c0 + y: the minimum of sum (n . y + d)^2 + lambda |y - (m - c0)|^2, continuous in its inputs, no rank test, condition number
 *      at most (1 + eps) / eps.  Then x is clamped, component by component in float64, to the cell's closed box
 *      [origin + q cell, origin + (q + 1) cell] and rounded to fp32 (which may leave it one ulp outside).
 *   5. Order of every sum: the float64 sums of rules 3, 4 and 7 run over lists sorted by (cluster, original index) -- the members of a
 *      cluster by packed vertex index, its corners by packed corner index 3 f + k -- in the order of "Fixed-order segmented sums" above,
 *      a cluster being a segment.  The ten quadric terms per corner are never stored: the corner pass reads the sorted corner list and
 *      forms n and d on the fly.  No floating-point atomics anywhere: two runs give the same bits.
 *   6. Faces: new face = (vert_map[v0], vert_map[v1], vert_map[v2]), same winding, kept iff its three new indices differ; kept faces stay
 *      in their original order; face_index (sum F') int64 points into the old packed face array.  Faces that come out equal are all kept.
 *   7. Attributes (sum V, C) fp32, 1 <= C <= 16: per cluster the mean of the members' rows, by the sums of rule 5, rounded to fp32.
 *
 * snr_simplify_keys: key (sum V) int64 of rule 2, 0 where rule 1 fails, and then *bad = 1 (device int32, zeroed by the caller).
 * snr_simplify_faces: new_faces (sum F, 3) int32 and keep (sum F) uint8 of rule 6 from vert_map; a face with an index outside its object
 *   reads nothing, gets (-1, -1, -1), keep 0, and *bad = 1.
 * snr_simplify_compact: out_faces (n_kept, 3), face_index (n_kept) from new_faces, keep and keep_scan (sum F) int64, the INCLUSIVE scan of
 *   keep along the packed faces; face f goes to slot keep_scan[f] - 1.
 * snr_simplify_positions: out_verts (n_clusters, 3) by rule 3 (quadric = 0) or rule 4 (quadric = 1).  vert_order (sum V) int64: the packed
 *   vertex indices sorted by (object, key), stable; vert_seg_start (n_clusters + 1) int64: cluster k's members at vert_order[vert_seg_start
 *   [k] .. vert_seg_start[k+1]), clusters of all objects packed object after object; vert_slab_offset (n_clusters + 1) int64: its slab
 *   offsets.  corner_order (3 sum F) int64: the corners 3 f + k sorted by the cluster of their vertex, stable, with
 *   corner_seg_start and corner_slab_offset alike (read only when quadric = 1 and sum F > 0).  vert_partial (n_vert_slabs, 3) and
 *   corner_partial (n_corner_slabs, 9) float64 scratch, n_vert_slabs >= snr_segment_slab_bound(n_clusters, sum V), n_corner_slabs >=
 *   snr_segment_slab_bound(n_clusters, 3 sum F), else SNR_E_WORKSPACE.  The cell of a cluster is rule 1
 *   applied to its first member.  Every index read from a list is range-checked before use; an entry out of range adds nothing.
 * snr_simplify_attributes: out (n_clusters, C) of rule 7 on the same vertex segments; partial (n_slabs, C) float64 scratch.
 * A null pointer, a negative size, n_clusters > sum V or C outside [1, 16]: SNR_E_ARG; more than 2^38 vertices or faces, or 2^31 clusters
 * or slabs, in a launch: SNR_E_UNSUPPORTED. */
#define SNR_SIMPLIFY_EPS 1e-3 /* rule 4's ridge weight: a design constant, not a tolerance */
int snr_simplify_keys(const float* verts, const int64_t* vert_offset, const float* cell, const float* origin, int64_t n_objects,
                      int64_t n_verts, int64_t* key, int32_t* bad, void* stream);
int snr_simplify_faces(const int32_t* faces, const int32_t* vert_map, const int64_t* vert_offset, const int64_t* face_offset,
                       int64_t n_objects, int64_t n_verts, int64_t n_faces, int32_t* new_faces, uint8_t* keep, int32_t* bad, void* stream);
int snr_simplify_compact(const int32_t* new_faces, const uint8_t* keep, const int64_t* keep_scan, int64_t n_faces, int64_t n_kept,
                         int32_t* out_faces, int64_t* face_index, void* stream);
int snr_simplify_positions(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset,
                           const float* cell, const float* origin, int64_t n_objects, int64_t n_verts, int64_t n_faces,
                           const int64_t* vert_order, const int64_t* vert_seg_start, const int64_t* vert_slab_offset,
                           const int64_t* corner_order, const int64_t* corner_seg_start, const int64_t* corner_slab_offset,
                           int64_t n_clusters, int quadric, double* vert_partial, int64_t n_vert_slabs, double* corner_partial,
                           int64_t n_corner_slabs, float* out_verts, void* stream);
int snr_simplify_attributes(const float* attributes, int n_channels, int64_t n_verts, const int64_t* vert_order,
                            const int64_t* vert_seg_start, const int64_t* vert_slab_offset, int64_t n_clusters, double* partial,
                            int64_t n_slabs, float* out, void* stream);

/* Mesh smoothing: which vertices of a packed mesh are neighbours, and Jacobi smoothing steps over that adjacency (Taubin 1995).  The mesh is
 * the packed form of "Mesh components" above (verts (sum V, 3) fp32, object-local int32 faces, vert_offset and face_offset DEVICE arrays).
 * tests/smooth_restatement.py restates every rule in numpy, one function each.
 *   1. Neighbours: in one object, j is a neighbour of i iff i != j and some face whose three indices all lie in [0, V) names both.
 *      Connectivity is by INDEX, not by position.  A face with a repeated index gives the pairs of its distinct indices; a face with an
 *      index outside [0, V) gives nothing and sets *bad.  Each neighbour counts once, however many faces name the pair; a vertex no face
 *      names has degree 0.
 *   2. Adjacency: a CSR over all vertices of the call -- nbr_start (sum V + 1) int64; nbr (E2) int32, LOCAL indices, ascending within each
 *      vertex; edge_faces (E2) int32 = how many faces name the undirected edge {i, j} (a face names an edge at most once; both directions
 *      of an edge carry the same count).  d_i = nbr_start[i + 1] - nbr_start[i] is the degree.  It comes from the caller's sort of the
 *      keys of snr_smooth_edge_keys: six per face, (global source index) * 2^31 + (local target index) for both directions of each of the
 *      face's distinct edges, INT64_MAX for a discarded pair; a neighbour is a run of equal keys, edge_faces the run's length.
 *   3. Classes: an edge with edge_faces == 1 is a boundary edge, one with edge_faces > 2 is non-manifold; a vertex is a boundary
 *      (non-manifold) vertex iff one of its edges is.  Two identical faces make their edges count 2.
 *   4. Umbrella operator on C <= 16 channels x (sum V, C) fp32 (positions: C = 3), per channel in float64:
 *          s = 0.0;  for j over N(i) ASCENDING: s += (double) x_j;   U_i = s / (double) d_i - (double) x_i;   U_i = 0 where d_i = 0.
 *      The library is built without fused multiply-adds and nothing is added atomically: every operation is one correctly rounded IEEE
 *      operation and the order is part of the contract (one thread per vertex walks its list; no wave-level reduction).
 *   5. Step: x'_i = (float)((double) x_i + f * U_i), f a double.  A pinned vertex (pinned[i] != 0) and a vertex of degree 0 keep their
 *      bits; a pinned vertex still serves as a neighbour.  A Jacobi step: x_out must not overlap x_in, else SNR_E_ARG.  Non-finite values
 *      are not tested for: a NaN vertex poisons exactly its 1-ring per step.
 *   6. Taubin lambda|mu: one iteration = a step with f = lambda, then a step with f = mu on the RESULT of the first (U computed anew).
 *      lambda = 0.5, mu = -0.53 (pass-band 0.1) neither shrink nor grow a closed shape much; without the mu step it is plain Laplacian
 *      smoothing, which shrinks.  (Host policy: two buffers, one launch per half-step, nothing read back.)
 *   7. Operator and transpose: transpose = 0 writes (float) U_i.  transpose = 1, of a gradient g (sum V, C):
 *          t = 0.0;  for j over N(i) ASCENDING: t += (double) g_j / (double) d_j;   out_i = (float)(d_i > 0 ? t - (double) g_i : t).
 *      The adjacency is symmetric, so both are gathers over the same CSR: no scatter, no atomics.
 *
 * snr_smooth_edge_keys: key (6 sum F) int64 of rule 2, face f's at key[6 f .. 6 f + 6); *bad (device int32, zeroed by the caller) = 1 if a
 *   face index lies outside its object.  Takes sum V < 2^32 (the key keeps 32 bits of source), else SNR_E_UNSUPPORTED.
 * snr_smooth_vertex_flags: boundary, nonmanifold (sum V) uint8 of rule 3 from nbr_start and edge_faces.
 * snr_smooth_step: x_out (sum V, C) of rule 5 from x_in; pinned (sum V) uint8 or NULL (nothing pinned).
 * snr_smooth_laplacian: out (sum V, C) of rule 7 from x; out must not overlap x.
 * Every neighbour index and every nbr_start pair is range-checked before use (an entry out of range adds nothing; a vertex whose pair is
 * not usable has degree 0).  A null pointer, a negative size, C outside [1, 16], transpose other than 0 / 1 or overlapping buffers:
 * SNR_E_ARG; more than 2^38 vertices, faces, keys or CSR entries in a launch: SNR_E_UNSUPPORTED. */
int snr_smooth_edge_keys(const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, int64_t n_objects, int64_t n_verts,
                         int64_t n_faces, int64_t* key, int32_t* bad, void* stream);
int snr_smooth_vertex_flags(const int64_t* nbr_start, const int32_t* edge_faces, int64_t n_verts, int64_t n_edges, uint8_t* boundary,
                            uint8_t* nonmanifold, void* stream);
int snr_smooth_step(const float* x_in, int n_channels, const int64_t* nbr_start, const int32_t* nbr, const int64_t* vert_offset,
                    int64_t n_objects, int64_t n_verts, int64_t n_edges, const uint8_t* pinned, double factor, float* x_out, void* stream);
int snr_smooth_laplacian(const float* x, int n_channels, const int64_t* nbr_start, const int32_t* nbr, const int64_t* vert_offset,
                         int64_t n_objects, int64_t n_verts, int64_t n_edges, int transpose, float* out, void* stream);

/* Mesh rasteriser: which face of a packed triangle mesh each pixel of a pinhole camera sees, at which depth and with which barycentric
 * weights.  The mesh is the packed form of "Mesh components" above (verts, object-local int32 faces, vert_offset and face_offset DEVICE
 * arrays).  Each object b has one row-major 3x4 fp32 matrix M_b (obj_to_cam (n_objects, 3, 4), DEVICE) that maps its stored vertices to
 * the camera frame (x right, y down, z forward); the camera is fx, fy, cx, cy.  All fp32 steps round once per written operation (no fma);
 * tests/raster_restatement.py restates every rule step by step.
 *   1. Projection of a vertex (x, y, z): per axis k, Xc_k = ((M[k][0] x + M[k][1] y) + M[k][2] z) + M[k][3]; its screen vertex is
 *      u = fx (Xc_0 / Xc_2) + cx, v = fy (Xc_1 / Xc_2) + cy, with the camera depth Xc_2 kept beside it.  Pixel centres lie at INTEGER
 *      (u, v): pixel (px, py) looks along ((px - cx) / fx, (py - cy) / fy, 1).
 *   2. Snapping: xs = rint(256 u), ys = rint(256 v) (round half to even), integers with 8 sub-pixel bits.  A face is dropped when one of
 *      its vertices has a non-finite u, v or depth, a depth < z_near (z_near > 0), or |u| or |v| >= 2^22 pixels; so is a face with a vertex
 *      index outside its object, or of an object whose image index is outside [0, n_images).  Faces are NOT clipped against the near
 *      plane: a face that reaches behind z_near disappears whole.  The objects this is for lie in front of the camera.
 *   3. Orientation, exact in int64: A = (xs1 - xs0)(ys2 - ys0) - (xs2 - xs0)(ys1 - ys0); a face with A = 0 is dropped; s = sign(A).  The
 *      iso rules wind faces counter-clockwise seen from outside in a right-handed frame, so under an M_b of positive determinant a face
 *      seen from outside has A < 0 (y points down).  cull_sign (n_objects) int32, nullable: a face with A cull_sign[b] > 0 is dropped;
 *      sign(det M_b[:, :3]) there drops the faces seen from inside, 0 (or a null array) draws both sides.
 *   4. Coverage, exact in int64, of the pixel centre P = (256 px, 256 py): edge i runs from vertex a = i + 1 to b = i + 2 (mod 3), the edge
 *      opposite vertex i; (dx, dy) = s (b - a); E_i = dx (P_y - a_y) - dy (P_x - a_x).  The pixel is covered iff for all three edges
 *      E_i > 0, or E_i = 0 and the edge owns its ties: dy > 0, or dy = 0 and dx < 0.  Two faces on opposite sides of a shared edge see it
 *      in opposite directions, so exactly one of them owns a centre on it.  Candidates are the pixels of the snapped bounding box inside
 *      [0, W - 1] x [0, H - 1].  (Coordinates stay within 2^30, differences within 2^31: every product fits int64.)
 *   5. Depth of a covered pixel: iz_i = 1.0f / z_i; q = (float(E_0) iz_0 + float(E_1) iz_1) + float(E_2) iz_2; depth = float(s A) / q, int64
 *      to float rounding to nearest even.  It is the perspective-correct camera z; every term is positive (E_0 + E_1 + E_2 = s A).
 *   6. Visibility: per pixel the covering face of smallest depth wins, ties to the smallest packed face index: the 64-bit key
 *      (bits(depth) << 32) | packed face (depth > 0: its bits order like its value), combined by UNSIGNED integer atomic min into keys
 *      (n_images, H, W), preset by the caller to all ones.  The result does not depend on the order of the threads.  Object b is drawn
 *      into image image_of_object[b] (int32, DEVICE): all zeros = one scene image, 0, 1, 2 ... = one image per object.
 *   7. Resolve, per pixel: face = the packed index (int32), -1 where empty; depth, 0 where empty; weights_i = (float(E_i) iz_i) / q
 *      recomputed for the winning face, the perspective-correct barycentric weights, 0 where empty.
 *   8. Interpolation of per-vertex attributes (sum V, C) fp32, 1 <= C <= 16: out_c = (w_0 a_0c + w_1 a_1c) + w_2 a_2c with a_i the row of
 *      the winning face's vertex i; an empty pixel gets `background`.
 *
 * snr_raster_project: screen (sum V, 3) = (u, v, Xc_2) of every vertex (rule 1), a thread per vertex.
 * snr_raster_faces: rules 2 - 6, a thread per face walking its candidate box; a face with 64 candidates or more is walked by its whole wave,
 *   64 pixels at a time.  Vector integer atomics only; no key is read in this launch (the L2s of the eight XCDs are not coherent
 *   within one).
 * snr_raster_resolve (a later launch: plain loads of keys): face (n_images, H, W) int32, depth (n_images, H, W), weights (n_images, H, W, 3).
 * snr_raster_interpolate: out (n_pixels, C) from face (n_pixels) and weights (n_pixels, 3), a thread per pixel and channel.
 * A null pointer, a negative size, z_near <= 0 or C outside [1, 16]: SNR_E_ARG; n_images H W >= 2^31 or sum F >= 2^31: SNR_E_UNSUPPORTED. */
int snr_raster_project(const float* verts, const int64_t* vert_offset, int64_t n_objects, int64_t n_verts, const float* obj_to_cam, float fx,
                       float fy, float cx, float cy, float* screen, void* stream);
int snr_raster_faces(const float* screen, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset,
                     const int32_t* image_of_object, const int32_t* cull_sign, int64_t n_objects, int64_t n_verts, int64_t n_faces,
                     int64_t n_images, int height, int width, float z_near, uint64_t* keys, void* stream);
int snr_raster_resolve(const uint64_t* keys, const float* screen, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset,
                       int64_t n_objects, int64_t n_verts, int64_t n_faces, int64_t n_images, int height, int width, int32_t* face,
                       float* depth, float* weights, void* stream);
int snr_raster_interpolate(const int32_t* face, const float* weights, const int32_t* faces, const int64_t* vert_offset,
                           const int64_t* face_offset, int64_t n_objects, int64_t n_verts, int64_t n_faces, const float* attributes,
                           int n_channels, int64_t n_pixels, float background, float* out, void* stream);

/* Mesh painting: per-vertex colours of a packed mesh from the photographs of its views.  Each vertex takes its colour from the views that
 * really see it, weighed by how squarely they face it; what no view sees is filled from its neighbours.  One view per launch: `screen`
 * (sum V, 3) is snr_raster_project's (u, v, camera z) for that view (rule 1 of "Mesh rasteriser": pixel centres at INTEGER (u, v)),
 * `depth` (H, W) snr_raster_resolve's for the same view (0 where empty), `image` (H, W, 3) fp32 the photograph on the same pixel grid,
 * `mask` (H, W) fp32 or NULL its occupancy (> 0: the object; 0 background, -1 another object in front).  All fp32 steps round once per
 * written operation (no fma), in the written order; tests/paint_restatement.py restates every rule step by step.
 *   P1. Footprint.  A vertex is skipped when u, v or z is not finite, z < z_near, u < 0, v < 0, u > float(W - 1) or v > float(H - 1).
 *       Otherwise x0 = min(int(floor(u)), W - 2) and a = u - float(x0) (exact); with W = 1, x0 = 0 and a = 0; y0 and b likewise from v and
 *       H.  The four taps, in this order, and their weights: (x0, y0) (1 - a)(1 - b); (x0 + 1, y0) a (1 - b); (x0, y0 + 1) (1 - a) b;
 *       (x0 + 1, y0 + 1) a b -- one subtraction and one product each.  With W = 1 (H = 1) the taps at x0 + 1 (y0 + 1) would repeat
 *       their neighbour: they are not read and are never valid.  So u = W - 1 exactly has x0 = W - 2 and a = 1.
 *   P2. Valid taps.  A tap is valid iff depth there > 0, and mask there > 0 when a mask is given, and z <= depth + tol (one fp32 add, one
 *       compare; false on a NaN).  s = the sum of the valid taps' weights in tap order, STARTING FROM the first valid term (not from 0);
 *       the view's colour per channel c = (sum over the valid taps of w_t I_t, same order, same start) / s, one division.  Only valid taps
 *       enter: the whitened background and occluders stay out of silhouette vertices, and the rest is renormalised.  The vertex is seen
 *       by the view only if s > 0.
 *   P3. Facing.  Without normals g = 1.  With normals n (sum V, 3) and the stored vertex x: d = centre - x (the camera centre in the
 *       frame of the stored vertices); dot = (n0 d0 + n1 d1) + n2 d2; nn and dd likewise of n with n and d with d; g = (dot dot) / (nn dd)
 *       when dot > 0 and nn dd is finite and > 0, else 0: cos^2 of the angle, no square root.  A view with g = 0 (or a g that is not > 0)
 *       does not see the vertex.
 *   P4. Accumulate, for a vertex the view sees (P1, s > 0, g > 0), plain in-place fp32 operations: sum_rgb_j = sum_rgb_j + g c_j (one
 *       product, one add); sum_w = sum_w + g; seen = seen + 1; if g > best_w (strict: ties keep the earlier view): best_w = g, best =
 *       view, best_rgb = c.  The caller presets sum_rgb, sum_w, best_w, best_rgb to 0, seen to 0 and best to -1 and launches the views in
 *       ascending order on one stream: that order is the order of the sums.  A vertex the view does not see has nothing written.
 *   P5. Finish.  Where seen > 0: colors_j = sum_rgb_j / sum_w (blend 0, "weighted": one division) or best_rgb_j (blend 1, "best"), and
 *       filled = 0.  Elsewhere colors = background and filled = -1.
 *   P6. Fill, one Jacobi round r >= 1 between two buffers over the adjacency of "Mesh smoothing" (nbr_start, nbr; neighbours ascending):
 *       a vertex with filled < 0 that has at least one neighbour with filled >= 0 IN THE INPUT takes, per channel, in float64:
 *           s = 0.0;  for j over N(i) ASCENDING with filled_j >= 0: s += (double) c_j;   c_i = (float)(s / (double) count)
 *       and filled = r.  Every other vertex copies its colour (the same bits) and its filled.  After R rounds filled is the graph distance
 *       to the nearest seen vertex where that is <= R, and still -1 beyond.  The outputs must not overlap the inputs, else SNR_E_ARG.
 *
 * snr_paint_view: P1 - P4 for view `view` (>= 0), a thread per vertex, grid-stride; verts and normals (sum V, 3) or normals NULL (g = 1).
 * snr_paint_finish: colors (sum V, 3) and filled (sum V) int32 of P5; blend 0 reads sum_rgb and sum_w, blend 1 best_rgb.
 * snr_paint_fill: colors_out, filled_out of P6 from colors_in, filled_in; neighbour entries and nbr_start pairs are range-checked as in
 *   "Mesh smoothing".  No atomics, no LDS: the same bits from run to run.
 * A null pointer (but mask and normals), a negative size or view, z_near <= 0, a tol that is negative or not finite, blend outside {0, 1},
 * round < 1 or overlapping fill buffers: SNR_E_ARG; more than 2^38 vertices or CSR entries, or H W >= 2^31: SNR_E_UNSUPPORTED. */
int snr_paint_view(const float* screen, const float* verts, const float* normals, int64_t n_verts, const float* image, const float* mask,
                   const float* depth, int height, int width, float centre_x, float centre_y, float centre_z, float tol, float z_near,
                   int view, float* sum_rgb, float* sum_w, int32_t* seen, float* best_w, int32_t* best, float* best_rgb, void* stream);
int snr_paint_finish(const float* sum_rgb, const float* sum_w, const int32_t* seen, const float* best_rgb, int64_t n_verts, int blend,
                     float background, float* colors, int32_t* filled, void* stream);
int snr_paint_fill(const float* colors_in, const int32_t* filled_in, const int64_t* nbr_start, const int32_t* nbr, const int64_t* vert_offset,
                   int64_t n_objects, int64_t n_verts, int64_t n_edges, int round, float* colors_out, int32_t* filled_out, void* stream);

/* Mesh distance: the closest point of a packed triangle mesh to a query point, and area-uniform samples of its surface.  The mesh is the
 * packed form of "Mesh components" above (verts fp32, object-local int32 faces, vert_offset and face_offset DEVICE arrays).  Queries are
 * packed the same way: points (sum Q, 3) fp32 with query_offset (n_objects + 1) int64, DEVICE; a query of object b sees the faces of
 * object b only.  The library is built without fused multiply-adds: all arithmetic of D1 - D3 is float64 on the widened fp32 inputs, one
 * correctly rounded float64 operation per written operation, in the written order.  tests/nearest_restatement.py restates every rule in
 * numpy, one function each; the kernels give its bits.
 *   D1. Point - triangle: the closest point of (a, b, c) to p by the region walk of Ericson (Real-Time Collision Detection, 5.1.5), in
 *       differences only, so that no rounding error grows with the distance of the object from the origin.  With dot(x, y) = (x0 y0 +
 *       x1 y1) + x2 y2:  ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c;  d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp),
 *       d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp);  vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4.  The first
 *       test that holds decides, in this order (weights w of a, b, c; e = p - closest point):
 *         vertex a:  d1 <= 0 and d2 <= 0:                                         w = (1, 0, 0),          e = ap;
 *         vertex b:  d3 >= 0 and d4 <= d3:                                        w = (0, 1, 0),          e = bp;
 *         edge ab:   vc <= 0, d1 >= 0, d3 <= 0 and d1 - d3 > 0:  t = d1 / (d1 - d3),  w = (1 - t, t, 0),  e = ap - t ab;
 *         vertex c:  d6 >= 0 and d5 <= d6:                                        w = (0, 0, 1),          e = cp;
 *         edge ac:   vb <= 0, d2 >= 0, d6 <= 0 and d2 - d6 > 0:  t = d2 / (d2 - d6),  w = (1 - t, 0, t),  e = ap - t ac;
 *         edge bc:   va <= 0, g = d4 - d3 >= 0, h = d5 - d6 >= 0 and g + h > 0:  t = g / (g + h),  w = (0, 1 - t, t),  e = bp - t (c - b);
 *         interior:  s = (va + vb) + vc,  v = vb / s,  u = vc / s,  w = ((1 - v) - u, v, u),  e = (ap - v ab) - u ac.
 *       d^2 = (ex^2 + ey^2) + ez^2.  An edge test also asks for a positive denominator, so no quotient is 0 / 0: a face without area
 *       (coincident corners; exactly collinear corners in either order) needs no other care and gives the distance to its segment or
 *       point.  Should rounding still leave s = 0 in the last line, d^2 is not finite; a candidate whose d^2 is NaN or +inf never wins.
 *   D2. The answer is the brute-force one: over all faces of the query's object the face with the smallest d^2 wins, ties to the lowest
 *       face index.  A face with an index outside [0, V) is skipped and sets *bad; a face with a vertex coordinate that is not finite is
 *       skipped.  A query with a non-finite coordinate, or an object without a usable face, gets face -1, weights 0 and d^2 = +inf.  The
 *       grid below may only change how many faces are tested; it may never change the result.
 *   D3. The grid.  Object b has cubic cells of edge h = cell[b] > 0 (fp32, widened), anchored at lo = grid_lo[b], the exact fp32 minimum
 *       of its vertices; grid_hi[b] is their exact maximum (both (n_objects, 3) fp32; 0 for an object without vertices).  Per axis
 *       n_a = clamp(ceil((hi_a - lo_a) / h), 1, 256) cells; the cell of a coordinate x is clamp(floor((x - lo_a) / h), 0, n_a - 1), so
 *       border cells reach to infinity outwards.  A face is listed in every cell of the index box spanned by the cells of its component-
 *       wise minimum and maximum corner.  Cell (cx, cy, cz) of object b has the id cell_offset[b] + (cx n_y + cy) n_z + cz; cell_offset
 *       (n_objects + 1) int64 = the exclusive scan of n_x n_y n_z, n_cells its last entry.  An object whose h is not positive and finite,
 *       whose bounds are not finite or whose cell_offset entries do not hold exactly its n_x n_y n_z cells has no usable grid: *bad.
 *   D4. The search, one thread per query.  c0 = the cell of the query.  For r = 0, 1, ...: visit the cells at Chebyshev distance r from
 *       c0 that lie inside the grid and test every listed face by D1 and D2 (a face listed in several cells is tested again: harmless).
 *       After ring r, with t_a = p_a - lo_a:  m = the smallest of t_a - k h over the axes with k = c0_a - r >= 1 and of k h - t_a over
 *       the axes with k = c0_a + r + 1 <= n_a - 1 -- the distance to the bounding planes of the block [c0 - r, c0 + r] on the sides
 *       where the grid goes on.  No such side: the search is over.  Otherwise stop iff
 *           s = m - 2^-40 (E + m) > 0  and  s s > best d^2,        E = the largest hi_a - lo_a of the object.
 *       Why this cannot change the result: a face not yet tested has no cell in the block, so on some axis all of its vertices fall
 *       into cells beyond one of those planes; the cell function is monotone, so every point of the face lies beyond the plane up to the
 *       rounding of (x - lo) / h and of k h, a few 2^-53 of E; the e of D1 is formed from differences whose roundings are a few 2^-53
 *       of |p - a| <= E + m + the distance found.  The slack 2^-40 (E + m) is 2^12 times all of that, and 2^-16 of the fp32 resolution
 *       of the inputs, so it costs no measurable extra ring.  The part 2^-40 E covers queries near the object, the part 2^-40 m queries
 *       far from it, whose roundings grow with their distance and not with E.  A face that only ties the best (equal d^2, lower index)
 *       is beyond no plane by more than the slack either, so it is still visited.
 *   D5. Surface samples.  Sample i of the n samples of an object takes three uniforms u (3) float64 in [0, 1) -- an input, as the render
 *       path takes injected jitter -- and the object's INCLUSIVE cumulative face area cum (F) float64, an input too (the face-area term
 *       is rule 3 of "Mesh components"; the scan is the caller's).  target = ((double) i + u0) / (double) n * cum[F - 1]; the face is
 *       the first f with cum[f] > target, or, where rounding leaves none, the first f with cum[f] >= cum[F - 1]: the last face with
 *       area.  So a face without area is never chosen.  s = sqrt(u1), correctly rounded; weights (1 - s, s (1 - u2), s u2); the point
 *       is (w0 a + w1 b) + w2 c per coordinate in float64, rounded once to fp32; the weights are rounded to fp32.  The draw is
 *       stratified: the number of samples on a face differs from n area_f / area by less than 2.  An object with cum[F - 1] not
 *       positive and finite (or F = 0) gives face -1, weights 0, point 0; so does a chosen face with an index outside [0, V), with *bad.
 *
 * snr_nearest_count: count (sum F) int32 = the number of cells of D3 per face; 0 and *bad (device int32, zeroed by the caller) for a face
 *   with a bad index or a non-finite vertex, or of an object without a usable grid.
 * snr_nearest_emit: from count_scan (sum F) int64, the caller's EXCLUSIVE scan of those counts, the pairs pair_cell (n_pairs) int64 (global
 *   cell id) and pair_face (n_pairs) int32 (object-local face), face f's at count_scan[f] on; a slot outside [0, n_pairs) is not written.
 *   The caller sorts the pairs by cell with one stable sort and finds cell_start (n_cells + 1) int64 by a search over the sorted ids.
 * snr_nearest_query: face (sum Q) int32 (object-local, -1 for none), weights (sum Q, 3) fp32 and dist2 (sum Q) float64 by D1 - D4.  Every
 *   index read from a list is range-checked before use: a cell_start pair or a listed face out of range adds nothing.  The object of a
 *   query is found once, not per candidate face.
 * snr_surface_sample: points (sum S, 3) fp32, face (sum S) int32 and weights (sum S, 3) fp32 by D5; uniforms (sum S, 3) float64, cum_area
 *   (sum F) float64 (each object's own inclusive scan), sample_offset (n_objects + 1) int64.
 * Nothing is allocated, nothing is read back, the caller's stream is used; no atomics except the *bad flag.  A null pointer or a negative
 * size: SNR_E_ARG; more than 2^38 vertices, faces, queries, samples, cells or pairs in a launch: SNR_E_UNSUPPORTED. */
int snr_nearest_count(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, const float* cell,
                      const float* grid_lo, const float* grid_hi, const int64_t* cell_offset, int64_t n_objects, int64_t n_verts,
                      int64_t n_faces, int64_t n_cells, int32_t* count, int32_t* bad, void* stream);
int snr_nearest_emit(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, const float* cell,
                     const float* grid_lo, const float* grid_hi, const int64_t* cell_offset, const int64_t* count_scan, int64_t n_objects,
                     int64_t n_verts, int64_t n_faces, int64_t n_cells, int64_t n_pairs, int64_t* pair_cell, int32_t* pair_face,
                     void* stream);
int snr_nearest_query(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, const float* points,
                      const int64_t* query_offset, const float* cell, const float* grid_lo, const float* grid_hi, const int64_t* cell_offset,
                      const int64_t* cell_start, const int32_t* pair_face, int64_t n_objects, int64_t n_verts, int64_t n_faces,
                      int64_t n_queries, int64_t n_cells, int64_t n_pairs, int32_t* face, float* weights, double* dist2, int32_t* bad,
                      void* stream);
int snr_surface_sample(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, const double* cum_area,
                       const double* uniforms, const int64_t* sample_offset, int64_t n_objects, int64_t n_verts, int64_t n_faces,
                       int64_t n_samples, float* points, int32_t* face, float* weights, int32_t* bad, void* stream);

/* Mesh containment: on which side of a packed triangle mesh a point lies -- the integer winding number along +z, the signed number of
 * faces that the ray from p in direction +z crosses.  The mesh is the packed form of "Mesh components" above, the queries are packed as in
 * "Mesh distance" (points (sum Q, 3) fp32 with query_offset; a query of object b sees the faces of object b only), and the grid is the one
 * of "Mesh distance" D3, built by snr_nearest_count / snr_nearest_emit: there is no second index.  The iso rules wind faces counter-
 * clockwise seen from the low-density side ("Mesh components", rule 3), so for a closed mesh the value is the winding number of p: +1
 * inside a solid blob, 0 inside a closed cavity of it, 2 where two blobs overlap, 0 outside.  A mesh that the border of the grid cut open
 * gets the value of these rules and no more.  All arithmetic is float64 on the widened fp32 inputs, one correctly rounded operation per
 * written operation, in the written order (the library is built without fused multiply-adds); compares of inputs are exact fp32 compares.
 * tests/inside_restatement.py restates every rule in numpy, one function each; the kernels give its integers.
 *   W1. Box guard.  Face (a, b, c) can count for p only if  min x <= p_x < max x,  min y <= p_y < max y  and  p_z < max z  over its three
 *       corners.  The guard is part of the rule, not an optimisation: it is what makes pruning by a grid unable to change the answer (W5).
 *   W2. Edge side, the same bits from both faces of an edge.  For the directed edge u -> v let (u', v') be the two endpoints ordered
 *       lexicographically by (x, y):  E = (v'_x - u'_x) (p_y - u'_y) - (v'_y - u'_y) (p_x - u'_x);  s = sign(E); if 0, s = sign(-(v'_y -
 *       u'_y)); if still 0, s = sign(v'_x - u'_x); if still 0 (a projected edge without length), s = 0.  s is negated if the endpoints
 *       were swapped.  This takes the query as (p_x + e, p_y + e^2) with e -> 0+: a point exactly under an edge or a vertex belongs to
 *       exactly one of the faces around it.  For fp32 inputs of comparable magnitude the differences and products are exact in float64,
 *       so the sign is exact; the canonical order makes the two faces of an edge evaluate the same expression, so they agree on the side
 *       even where rounding makes it wrong.
 *   W3. Crossing.  sigma = s(a -> b).  The face's column contains p iff  s(a -> b) = s(b -> c) = s(c -> a) != 0.  sigma = +1: the
 *       projection is counter-clockwise, the normal has a +z component.  A face without projected area (vertical, or without area at
 *       all) never counts.
 *   W4. Ahead.  n = (b - a) x (c - a), each component x1 y2 - x2 y1 as written:  n_x = (b_y - a_y)(c_z - a_z) - (b_z - a_z)(c_y - a_y),
 *       n_y = (b_z - a_z)(c_x - a_x) - (b_x - a_x)(c_z - a_z),  n_z = (b_x - a_x)(c_y - a_y) - (b_y - a_y)(c_x - a_x).
 *       t = (n_x (a_x - p_x) + n_y (a_y - p_y)) + n_z (a_z - p_z).  The face is ahead of p iff sigma t > 0: no division.  t = 0 (p on the
 *       face's plane) is not ahead, so a point on the surface is not under that face.  The face contributes sigma.
 *   W5. The answer is the brute-force one: winding(p) = the sum over ALL faces of p's object of the contributions, int32.  A face with an
 *       index outside [0, V) is skipped and sets *bad; a face with a vertex coordinate that is not finite is skipped.  A query with a
 *       non-finite coordinate, and every query of an object without a usable grid (D3; *bad), gets 0.  Pruning: a thread walks the
 *       z-column of cells (c_x(p), c_y(p), k), k = c_z(p) .. n_z - 1 -- contiguous entries of cell_start, z being the fastest cell axis
 *       -- and a face listed in several cells of the column counts ONCE, in cell k = max(c_z(min z of the face), c_z(p)).  Why this
 *       cannot change the sum: the cell function of D3 is monotone and a face is listed in every cell of the index box of its corner
 *       cells; so min x <= p_x < max x gives c_x(min x) <= c_x(p) <= c_x(max x), likewise in y, and W1's guard puts every face that can
 *       count into this column of cells; and p_z < max z gives c_z(p) <= c_z(max z), so the chosen k lies between c_z(min z) and
 *       c_z(max z): the face is listed there, and there only is it counted.  A face not in the column fails W1 and contributes 0 in the
 *       brute force too.  The two integer comparisons use the very cell function the lists were built with.
 *   W6. Lattice form.  For a lattice of n = (n_x, n_y, n_z) points per object, point (i, j, k) is at lat_lo + lat_h index per axis: an
 *       fp32 multiply, then an fp32 add, rounded separately (the formula of the density lattices, "Geometry").  lat_lo and lat_h are
 *       (n_objects, 3) fp32 DEVICE arrays; n is shared.  The winding numbers are in the lattice's order (x-major, z fastest) and are THE
 *       SAME INTEGERS W1 - W5 give for those points.  W2, W3, n and the bracket of W4 do not depend on p_z, so a run of z-points of one
 *       column does them once per face, walking the column of cells from the cell of its lowest point; per z-point p_z < max z, the last
 *       multiply-add and the compare remain.
 *
 * snr_inside_query: winding (sum Q) int32 by W1 - W5, one thread per query; the mesh, the queries and the grid arrays exactly as
 *   snr_nearest_query takes them.  *bad (device int32, zeroed by the caller) as W5 says.
 * snr_inside_lattice: winding (n_objects n_x n_y n_z) int32 by W6; every entry is written, so the caller need not zero it.  One thread
 *   per 16 consecutive z-points of a column.
 * Every index read from a list is range-checked before use: a cell_start pair or a listed face out of range adds nothing.  Nothing is
 * allocated, nothing is read back, the caller's stream is used; no atomics except the *bad flag.  A null pointer or a negative size:
 * SNR_E_ARG; more than 2^38 vertices, faces, queries, cells, pairs or lattice points (per axis or in all) in a launch:
 * SNR_E_UNSUPPORTED.  Zero queries, zero objects of a lattice or a lattice without points: SNR_OK without a launch. */
int snr_inside_query(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, const float* points,
                     const int64_t* query_offset, const float* cell, const float* grid_lo, const float* grid_hi, const int64_t* cell_offset,
                     const int64_t* cell_start, const int32_t* pair_face, int64_t n_objects, int64_t n_verts, int64_t n_faces,
                     int64_t n_queries, int64_t n_cells, int64_t n_pairs, int32_t* winding, int32_t* bad, void* stream);
int snr_inside_lattice(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, const float* cell,
                       const float* grid_lo, const float* grid_hi, const int64_t* cell_offset, const int64_t* cell_start,
                       const int32_t* pair_face, const float* lat_lo, const float* lat_h, int64_t n_objects, int64_t n_verts, int64_t n_faces,
                       int64_t n_cells, int64_t n_pairs, int64_t n_x, int64_t n_y, int64_t n_z, int32_t* winding, int32_t* bad, void* stream);

/* Mesh ray casting: where a ray hits a packed triangle mesh first, and how many faces it crosses.  The mesh is the packed form of "Mesh
 * components" above; rays are packed as the queries of "Mesh distance" are (rays_o and rays_d (sum N, 3) fp32 with ray_offset (n_objects +
 * 1) int64, DEVICE; t_min and t_max (sum N) fp32; a ray of object b sees the faces of object b only), and the grid is the one of "Mesh
 * distance" D3, built by snr_nearest_count / snr_nearest_emit: there is no second index.  All arithmetic is float64 on the widened fp32
 * inputs, one correctly rounded operation per written operation, in the written order (the library is built without fused multiply-adds).
 * tests/raycast_restatement.py restates every rule in numpy, one function each; the kernels give its integers, its t bit for bit in
 * float64 and its weights bit for bit in fp32.
 *   R1. Ray frame (Woop, Benthin, Wald 2013, "Watertight ray/triangle intersection").  The ray is o + t d; d need not be unit, t is in
 *       units of |d|.  kz = the axis of the largest |d| (ties to the lowest axis); kx, ky = the next two axes cyclically, swapped when
 *       d[kz] < 0, so that winding is kept.  Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].  Per vertex v:  A = v - o;
 *       x' = A[kx] - Sx A[kz],  y' = A[ky] - Sy A[kz],  z' = Sz A[kz].  In (x', y', z') the ray is the z' axis and z' is its parameter.
 *       A ray with a non-finite component of o or d, or with d = 0, hits nothing and crosses nothing.
 *   R2. Edge side, the same bits from both faces of an edge: W2's construction on the projected corners, with the query at the origin.
 *       For the directed edge u -> v let (u', v') be the two endpoints ordered lexicographically by (x', y'):
 *       E = (v'_y - u'_y) u'_x - (v'_x - u'_x) u'_y  (W2's E with p = 0);  s = sign(E); if 0, s = sign(-(v'_y - u'_y)); if still 0,
 *       s = sign(v'_x - u'_x); if still 0, s = 0.  s AND E are negated if the endpoints were swapped.  This takes the ray through
 *       (e, e^2) of its own (x', y') plane with e -> 0+.  A shared vertex gives identical (x', y', z') in both faces, because the inputs
 *       and the operations are the same; so both faces of an edge evaluate the same expression, and a ray through a shared edge or
 *       vertex of a closed mesh crosses exactly one of the faces around it.
 *   R3. Crossing.  The ray's line crosses face (a, b, c) iff  s(a -> b) = s(b -> c) = s(c -> a) = sigma != 0.  A face seen edge-on or
 *       without area never counts.  sigma = -1 is FRONT-facing: the projection is clockwise seen against the ray, d . n < 0 with n =
 *       (b - a) x (c - a), the ray enters through the face.  sigma = +1 is back-facing: d . n > 0, the ray leaves through it (W3's
 *       sigma for d = +z).
 *   R4. Depth and weights.  U = E(b -> c), V = E(c -> a), W = E(a -> b), the values of the edges opposite a, b and c;  det = (U + V) +
 *       W;  t = ((U z'_a + V z'_b) + W z'_c) / det: the one division of a face, made after R3.  The weights of (a, b, c) are (U, V, W) /
 *       det, rounded to fp32.  The hit counts iff t_min < t < t_max, both strict (fp32 bounds, widened; t_max = +inf is allowed; a NaN
 *       t or bound never counts).  So a ray that starts on a face does not hit that face at t_min = 0: W4's "on the plane is not ahead".
 *   R5. The answers are the brute-force ones over ALL faces of the ray's object.  First hit: the counting face with the smallest t,
 *       ties to the lowest face index; face (int32, object-local, -1 for none), t (float64, +inf for none), weights (fp32, 0 for none),
 *       side (int8: +1 front, -1 back, 0 none).  cull = 0 keeps all faces, 1 drops back-facing faces, 2 drops front-facing faces,
 *       before the minimum is taken.  Crossings: signed (int32) = the sum of sigma over the counting faces (+1 where the ray leaves, -1
 *       where it enters), total (int32) = their number.  For a closed mesh wound as the iso rules wind it, signed of a ray to infinity
 *       is the winding number of its origin, in any direction, for an origin off the surface.  A face with an index outside [0, V) is
 *       skipped and sets *bad; a face with a vertex coordinate that is not finite is skipped; every ray of an object without a usable
 *       grid (D3; *bad) gets no hit and zero crossings: the treatment of D2 and W5.
 *   R6. Pruning, which may never change R5's answer.  With lo, hi and E the object's bounds and largest extent (D3) and m = the largest
 *       over the axes of lo_a - o_a, o_a - hi_a and 0, the slack is  s = 2^-40 (E + m)  and, as a parameter,  s_t = s / |d[kz]|.
 *       Clip:  [t_a, t_b] = [t_min, t_max] cut per axis with d_a != 0 to the parameters of lo_a - s and hi_a + s; an axis with d_a = 0
 *       and o_a outside [lo_a - s, hi_a + s], or t_a > t_b: the ray visits no cell.  Walk: slab k of cells along kz, from the cell of
 *       o[kz] + t_a d[kz] to that of o[kz] + t_b d[kz].  Its parameters: t_n, t_f of its near and far plane lo[kz] + k h; the interval
 *       [max(t_a, t_n - s_t), min(t_b, t_f + s_t)], with t_a for the first and t_b for the last slab (border cells reach outwards
 *       without end), and for the first hit cut at best t + s_t.  The other two coordinates at the interval's two ends span their
 *       range over it, the ray being linear; widened by s and taken through the cell function it gives the rectangle [i0, i1] x
 *       [j0, j1] of cells, kx outer, both ascending; kz is the dominant axis, so it is 2 x 2 cells at most but for the slack.  Every
 *       listed face of every cell of it is tested (again, if listed in several: harmless for the minimum).  First hit: stop after a
 *       slab once best t < t_f - s_t.  Crossings: a face counts ONCE, in slab  clamp(clamp(c_kz(o[kz] + t d[kz]), c_kz(min), c_kz(max)),
 *       the walk's slabs)  -- the slab of its hit, kept within the slabs that list the face -- and there in cell (max(i0, c_kx(min)),
 *       max(j0, c_ky(min))), the first cell of the rectangle that lists it (min, max: the face's corner extremes; c: D3's cell
 *       function, the one the lists were built with; W5's max(c_z(min z), c_z(p)) is the model).
 *       Why this cannot change the result: with lambda = (U, V, W) / det -- all of one sign, so a convex combination, whatever the
 *       roundings -- t is the combination of the z'_i, the ray's parameters of the corners' kz coordinates, and the hit point o + t d
 *       is the combination of the corners up to the roundings of R1's x', y' (a few 2^-53 of |v - o| <= E + m) and of U, V, W (a few
 *       2^-53 of the squared size of the projected face, over det).  So the hit point lies in the face's bounding box up to those, the
 *       box lies within the bounds, and a ray that misses the widened bounds has no hit; the cell function is monotone and a face is
 *       listed in every cell of the index box of its corner cells, so the cell of a point within s of the box lies within that index
 *       box when the point's coordinates are widened by s: the slab that holds parameter t visits a cell that lists the face.  A face
 *       not yet met when the first walk stops has its hit beyond the far plane less the slack, so a larger t; one that ties is within
 *       best t + s_t and is still met.  The slack is 2^12 times the roundings of well-conditioned faces and 2^-16 of the fp32
 *       resolution of the inputs.  The division by det is the one place where rounding can grow: a face as large as the whole object
 *       seen at less than 2^-9 rad from edge-on can exceed the slack; the rules give such a face the t of R4 in the brute force, and
 *       the walk may then differ.  Extracted meshes have faces of a cell of the lattice, where the bound is 2^-9 rad times face size
 *       over E.
 *
 * snr_raycast_first: face (sum N) int32, t (sum N) float64, weights (sum N, 3) fp32 and side (sum N) int8 by R1 - R6.
 * snr_raycast_crossings: signed_count and total (sum N) int32 by R1 - R6.
 * Both take the mesh and the grid arrays exactly as snr_nearest_query takes them, run one thread per ray and find the object of a ray
 * once; every index read from a list is range-checked before use (a cell_start pair or a listed face out of range adds nothing); every
 * output entry is written.  Nothing is allocated, nothing is read back, the caller's stream is used; no atomics except the *bad flag
 * (device int32, zeroed by the caller).  A null pointer, a negative size or a cull outside {0, 1, 2}: SNR_E_ARG; more than 2^38 vertices,
 * faces, rays, cells or pairs: SNR_E_UNSUPPORTED.  Zero rays: SNR_OK without a launch.  With zero faces and zero pairs the mesh and list
 * pointers may be null. */
int snr_raycast_first(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, const float* rays_o,
                      const float* rays_d, const int64_t* ray_offset, const float* t_min, const float* t_max, const float* cell,
                      const float* grid_lo, const float* grid_hi, const int64_t* cell_offset, const int64_t* cell_start,
                      const int32_t* pair_face, int64_t n_objects, int64_t n_verts, int64_t n_faces, int64_t n_rays, int64_t n_cells,
                      int64_t n_pairs, int cull, int32_t* face, double* t, float* weights, int8_t* side, int32_t* bad, void* stream);
int snr_raycast_crossings(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset,
                          const float* rays_o, const float* rays_d, const int64_t* ray_offset, const float* t_min, const float* t_max,
                          const float* cell, const float* grid_lo, const float* grid_hi, const int64_t* cell_offset,
                          const int64_t* cell_start, const int32_t* pair_face, int64_t n_objects, int64_t n_verts, int64_t n_faces,
                          int64_t n_rays, int64_t n_cells, int64_t n_pairs, int32_t* signed_count, int32_t* total, int32_t* bad,
                          void* stream);

/* ------------------------------------------------------------------------------------
 * Several views of one instance share one shape and one texture code (src/optimizer_nuscenes.py:796-1277): V rendered views, I <= V code
 * rows, the views of an instance contiguous (instance-major).
 *
 * snr_view_pixels: one iteration's random pixels of every view's native-resolution roi (render_rays, src/utils.py:380-432).  The V crops
 *   are concatenated row-major: view v's h_v x w_v pixels start at pixel crop_offset[v] of img (sum h w, 3) / occ (sum h w), which hold
 *   crop_offset[V] pixels (a pick is also refused where it leaves its view's slice crop_offset[v] .. crop_offset[v+1]);
 *   roi (V,4) int32 = x0 y0 x1 y1 with w = x1 - x0, h = y1 - y0; Kvec (V,4) = fx fy cx cy; picks (V,n) int32 = index y w + x into the
 *   view's crop.  Pick id is pixel x = x0 + id % w, y = y0 + id / w (get_rays' linspace(x0, x1 - 1, w) pixels, exact integers):
 *   cam_dirs (V,n,3) = ((x - cx) / fx, (y - cy) / fy, 1) with a correctly rounded fp32 division, rgb_tgt (V,n,3) and occ_out (V,n) gathered
 *   from the crop.  A pick outside [0, h w) (-1 by convention) is a PADDING ray: nothing is read, cam_dirs = (0,0,1), rgb_tgt = 0,
 *   occ_out = 0 -- which snr_loss_tail_* weighs with exactly 0 in every numerator and denominator, so a view with fewer than n pixels
 *   rides in the rectangular launch.  A thread per ray, striding beyond 262144 rays.
 * snr_instance_rows_fwd: src (I,C) -> dst (V,C), row v = the row of v's instance.  view_offset (I+1) int64 in DEVICE memory:
 *   instance i owns the views view_offset[i] .. view_offset[i+1]-1.  view_offset_host [nullable]: the same I+1 numbers in HOST memory,
 *   checked before the launch.
 * snr_instance_rows_bwd: d_dst (V,C) -> d_src (I,C): d_src[i,c] = the sum over the instance's views in ASCENDING order with plain fp32
 *   adds, starting from the first term; one thread per (i,c), no atomics: the same bits every run.
 * Any C >= 1.  SNR_E_ARG: a null pointer, I < 1, V < I, or host offsets that do not start at 0, end at V and ascend strictly (an
 * instance without a view).
 * ---------------------------------------------------------------------------------- */
int snr_view_pixels(const float* img, const float* occ, const int64_t* crop_offset, const int32_t* roi, const float* Kvec, const int32_t* picks,
                    int64_t n_views, int64_t n, float* cam_dirs, float* rgb_tgt, float* occ_out, void* stream);
int snr_instance_rows_fwd(const float* src, const int64_t* view_offset, const int64_t* view_offset_host, int64_t n_instances, int64_t n_views,
                          int64_t n_cols, float* dst, void* stream);
int snr_instance_rows_bwd(const float* d_dst, const int64_t* view_offset, const int64_t* view_offset_host, int64_t n_instances, int64_t n_views,
                          int64_t n_cols, float* d_src, void* stream);

/* ------------------------------------------------------------------------------------
 * Cross-view evaluation (OptimizerNuScenes.eval_cross_view, src/optimizer_nuscenes.py:1279-1410): the codes fitted to view ii of an instance,
 * rendered from the camera of view num and scored against view num's whitened crop and lidar returns.
 *
 * snr_cross_metrics: the rendered outputs of P (code row, target view) pairs -> out (P,3) = [mse_fg, depth_err, sum |occ|], one launch.
 *   rgb (P,n,3) and depth_pred (P,n_l): pair p's renders of the target view's n grid pixels and n_l (padded) lidar pixels;
 *   tgt (V,n,3), occ (V,n), lid_depth (V,n_l), lid_cnt (V) int32: the V views' resized targets, labels, measured depths and lidar
 *   counts; pairs (P,2) int32 in DEVICE memory = [code row, target view].  Pair p reads tgt / occ / lid_depth / lid_cnt THROUGH
 *   v = pairs[p][1]: nothing per-view is copied per pair (the code row is the caller's bookkeeping; the kernel does not read it).
 *     mse_fg    = sum_i ((rgb - tgt)^2 summed over the 3 channels) |occ_i| / (sum_i |occ_i| + 1e-9)              (:1359-1360)
 *     depth_err = sum_{k < lid_cnt[v]} |depth_pred[p,k] - lid_depth[v,k]| / (lid_cnt[v] + 1e-8)                   (:1378-1379)
 *   in fp32; lid_cnt is clamped to [0, n_l]; n_l == 0 (depth_pred, lid_depth, lid_cnt may be null): depth_err = 0.  A view whose occ is
 *   all zero gives mse_fg = 0 exactly.  One workgroup of 256 threads per pair, thread t owns the rays t + 256 k, fixed-order wave
 *   reduction, the 4 wave partials added in wave order through LDS, plain stores: no atomics, the same bits every run.
 *   pairs_host [nullable]: the same 2 P numbers in HOST memory, checked before the launch against n_codes and V.
 * SNR_E_ARG without a launch: a null pointer, P < 1, V < 1, n_codes < 1, n < 1, n_l < 0, or a host pair outside [0, n_codes) x [0, V).
 * ---------------------------------------------------------------------------------- */
int snr_cross_metrics(const float* rgb, const float* depth_pred, const float* tgt, const float* occ, const float* lid_depth,
                      const int32_t* lid_cnt, const int32_t* pairs, const int32_t* pairs_host, int64_t n_pairs, int64_t n_views, int64_t n_codes,
                      int64_t n, int64_t n_l, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUPNERF_HIP_H */
