/*
 * eslam_hip.h - C ABI of the MI355X (gfx950) implementation of ESLAM's per-iteration rendering hot path.
 *
 * The reference (MohammadJohari/myslam) is 100 % Python on PyTorch and has no FFI of its own; its boundary for
 * this path is the in-process Python API  Renderer.render_batch_ray / get_samples / Decoders.forward.
 * This header is the C-ABI a binding for that API calls (myslam_amd/_hip.py is the ctypes binding we ship,
 * INTEGRATION.md shows the stub a reference maintainer would add).  Each entry point names the reference
 * lines it replaces (paths relative to the reference repository root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to float32 / int64 data unless the name ends in _host;
 *   - `stream` is a hipStream_t (NULL = default stream); every call only enqueues work on it: no allocation,
 *     no synchronisation, no host<->device copy, so a caller may capture a call into a hipGraph;
 *   - return value 0 = ok, anything else = error; eslam_last_error() gives the message (thread local);
 *   - tri-planes are the reference's 6 lists x 2 levels flattened in `all_planes` order:
 *       index = 2*g + level,  g in (planes_xy, planes_xz, planes_yz, c_planes_xy, c_planes_xz, c_planes_yz),
 *     each a logical [1, C=32, h, w] tensor described by element strides, so both NCHW-contiguous tensors
 *     (what reference src/ESLAM.py:201-210 allocates) and channels-last ones (what myslam_amd.scene allocates;
 *     one texel = 128 contiguous bytes, the fast path) are accepted without a copy;
 *   - decoder parameters are the reference's tensors (src/networks/decoders.py:47-60), row-major [out, in].
 */
#ifndef ESLAM_HIP_H
#define ESLAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ESLAM_ABI_VERSION 5
#define ESLAM_C_DIM 32          /* feature channels per plane (configs/ESLAM.yaml:77)               */
#define ESLAM_HIDDEN 16         /* decoder hidden width (src/networks/decoders.py:39)               */
#define ESLAM_FEAT (2 * ESLAM_C_DIM)   /* coarse || fine                                          */
#define ESLAM_N_PLANES 12
#define ESLAM_MAX_SAMPLES 256   /* samples per ray supported by the per-ray kernels                  */
#define ESLAM_RAY_ORDERS 3      /* eslam_ray_order writes one order per plane orientation (xy, xz, yz)    */
#define ESLAM_RAY_ORDER_WORDS(R) (ESLAM_RAY_ORDERS * (int64_t)(R) + 4)   /* int32 words of its output buffer */
/* floats in the flat decoder-gradient vector, in the order of eslam_decoders_t (beta excluded)      */
#define ESLAM_N_DEC_PARAMS (2 * (16 * 64 + 16 + 16 * 16 + 16) + (1 * 16 + 1) + (3 * 16 + 3))

typedef void* eslam_stream_t;

typedef struct {
    const float* data;      /* element [0,0,0,0]                                                  */
    float* grad;            /* same strides as data; kernels ACCUMULATE (+=) into it; may be NULL  */
    int32_t h, w;
    int64_t stride_c, stride_y, stride_x;   /* in elements                                         */
    const void* data_f16;   /* optional IEEE-half copy of the plane, channels-last with the SAME element strides
                               (stride_c = 1, stride_x = 32: 64-byte texels).  When all 12 planes carry one, eslam_render_fwd*,
                               eslam_render_bwd* run the mixed-precision path of BASELINE.json configs[4]: texels gathered from
                               the half copies (float32 accumulation), decoders on bf16 MFMA forward AND backward, plane
                               gradients accumulated in float32 into `grad` (the float32 master's gradient), ray gradients
                               (g_rays_o / g_rays_d) from the bilinear derivative on the half texels.  The saved
                               features `feat` then hold R*S*128 bf16 values (half the bytes of the float32 path's buffer).
                               The free-point entries dispatch on it in the same way: eslam_decode_fwd (all three variants;
                               feat then [N,128] bf16), eslam_sdf_grid and eslam_decode_bwd (plane, decoder and point
                               gradients; g_pts from the bilinear derivative on the half texels).  In SDF-only mode the six
                               geometry planes decide.  All 12 planes carry a copy or none does.                        */
} eslam_plane_t;

typedef struct {            /* src/networks/decoders.py:47-60                                      */
    const float* w1;  const float* b1;      /* linears.0        [16,64],[16]                        */
    const float* w2;  const float* b2;      /* linears.1        [16,16],[16]                        */
    const float* w3;  const float* b3;      /* output_linear    [1,16],[1]                          */
    const float* cw1; const float* cb1;     /* c_linears.0      [16,64],[16]                        */
    const float* cw2; const float* cb2;     /* c_linears.1      [16,16],[16]                        */
    const float* cw3; const float* cb3;     /* c_output_linear  [3,16],[3]                          */
    const float* beta;                      /* [1] (a device copy of the int when not learnable)    */
} eslam_decoders_t;

const char* eslam_last_error(void);
int eslam_abi_version(void);

/* K1 - pixel pick + back-projection.  Replaces src/common.py:87-153 (get_samples and helpers) with the
 * torch.randint draw of common.py:108 lifted to the caller: indices[b*n] are flat positions inside the crop
 * window [H0,H1) x [W0,W1), row-major, image k owning indices[k*n .. (k+1)*n).
 * depths [b,H,W], colors [b,H,W,3] contiguous; c2ws [b,4,4] row-major.
 * Outputs rays_o/rays_d [b*n,3], depth [b*n], color [b*n,3].                                        */
int eslam_sample_rays(const int64_t* indices, int b, int n, int H0, int H1, int W0, int W1, int H, int W,
                      float fx, float fy, float cx, float cy, const float* c2ws, const float* depths,
                      const float* colors, float* rays_o, float* rays_d, float* depth, float* color,
                      eslam_stream_t stream);

/* Backward of K1 w.r.t. the camera matrices (autograd of common.py:92-97): g_c2ws [b,4,4] is OVERWRITTEN
 * with  d/dc2w ( <g_rays_o, rays_o> + <g_rays_d, rays_d> );  rows/cols outside [:3,:4] are zero.     */
int eslam_sample_rays_bwd(const int64_t* indices, int b, int n, int H0, int W0, int W1, float fx, float fy,
                          float cx, float cy, const float* g_rays_o, const float* g_rays_d, float* g_c2ws,
                          eslam_stream_t stream);

/* Whole-image rays.  Replaces src/common.py:183-201 (get_rays).  rays_o/rays_d [H*W,3].             */
int eslam_image_rays(int H, int W, float fx, float fy, float cx, float cy, const float* c2w, float* rays_o,
                     float* rays_d, eslam_stream_t stream);

/* a2 - AABB exit distance  min_axis max_side (bound - o)/d.  Replaces the caller-side pre-filter arithmetic
 * of src/Mapper.py:322-328 and src/Tracker.py:175-181.  t_exit [R].                                  */
int eslam_aabb_exit(const float* rays_o, const float* rays_d, int R, const float* bound6_host, float* t_exit,
                    eslam_stream_t stream);

/* K3 - depth-guided sampler.  Replaces src/utils/Renderer.py:85-105 and perturbation (:46-61) for rays with
 * gt_depth > 0; rows of rays with gt_depth <= 0 are left untouched (K4 fills them).
 * t_free[n_strat], t_surf[n_imp]: the two linspace(0,1,.) vectors (device); t_rand [R,S] uniform numbers or
 * NULL for perturb = False.  z_vals [R,S] out, S = n_strat + n_imp.  Bit-exact vs the reference arithmetic
 * (truncation is a double because Renderer.py:97 forms 1.5*truncation and 3*truncation as Python floats).    */
int eslam_sample_z(const float* gt_depth, int R, int n_strat, int n_imp, double truncation, const float* t_free,
                   const float* t_surf, const float* t_rand, float* z_vals, eslam_stream_t stream);

/* K4 - importance sampler for rays with gt_depth <= 0.  Replaces src/utils/Renderer.py:108-134 and
 * src/common.py:41-77 (sample_pdf, det=False).  Only geometry planes + SDF decoder are evaluated, no grad.
 * t_rand_uni [R,n_strat] or NULL, u [R,n_imp]; rows of rays with gt_depth > 0 are ignored / left untouched. */
int eslam_importance_z(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                       const float* rays_o, const float* rays_d, const float* gt_depth, int R, int n_strat,
                       int n_imp, const float* t_free, const float* t_rand_uni, const float* u, float* z_vals,
                       eslam_stream_t stream);

/* eslam_sample_z + eslam_importance_z in ONE launch: every row of z_vals [R, n_strat+n_imp] - rays with gt_depth > 0 by
 * the depth-guided rule (bit-exact, as eslam_sample_z), the others by the importance sampler.  Needs n_strat >= 3.    */
int eslam_sample_z_all(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                       const float* rays_o, const float* rays_d, const float* gt_depth, int R, int n_strat, int n_imp,
                       double truncation, const float* t_free, const float* t_surf, const float* t_rand,
                       const float* t_rand_uni, const float* u, float* z_vals, eslam_stream_t stream);

/* eslam_sample_z_all with the random numbers drawn INSIDE the kernel instead of read from t_rand / t_rand_uni / u (the
 * reference draws them with torch.rand, Renderer.py:59 and common.py:59; a caller that needs the reference's exact
 * stream injects it through eslam_sample_z_all): U = hash(seed, step, stream, element) / 2^24 in [0,1), with
 * step = *rng_state (device memory; NULL = 0).  perturb = 0 leaves the samples un-jittered (Renderer.perturb False);
 * the importance draw is random either way.  Pass the same rng_state as `rng_bump` to the eslam_render_fwd* call that
 * consumes z_vals: it advances the step, so a replayed hipGraph draws fresh numbers without an extra launch.
 * ray_offset: index of this call's ray 0 in the iteration's whole batch (0 for an unsharded call).  The numbers are keyed
 * on the GLOBAL ray index ray_offset + i, so the ranks of a ray-sharded iteration - same seed, same step - draw exactly what
 * the unsharded batch draws: its z_vals, and with them the loss's set sizes, do not depend on the world size.            */
int eslam_sample_z_all_rng(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                           const float* rays_o, const float* rays_d, const float* gt_depth, int R, int n_strat, int n_imp,
                           double truncation, const float* t_free, const float* t_surf, int perturb, uint64_t seed,
                           const uint32_t* rng_state, int64_t ray_offset, float* z_vals, eslam_stream_t stream);

/* K5-K7 forward.  Replaces src/utils/Renderer.py:136-147 + src/networks/decoders.py:64-146 +
 * src/common.py:204-218:  pts = o + d z -> normalise -> tri-plane bilinear gather (border, align_corners) ->
 * SDF / colour MLPs -> sdf2alpha -> transmittance scan -> composite.
 * Outputs: depth [R], rgb [R,3], sdf [R,S].  For a later backward pass also raw_rgb [R,S,3] (sigmoid outputs)
 * and feat [R*S,128] (geometry 64 || colour 64 features per sample); both may be NULL for inference.  With feat given,
 * R*S is limited to 8 388 607 points (rows of feat, and of the backward pass's feature-gradient buffer, are addressed with
 * 32-bit byte offsets: R*S*512 < 2^32 - 256); larger batches return an error - split them (inference has no such limit).
 * ray_order [ESLAM_RAY_ORDERS][R] (optional, from eslam_ray_order; the forward uses the first): the kernel walks the rays in that order with an XCD-contiguous
 * block mapping; outputs stay in the caller's ray order.  NULL = rays are processed as given, which measured FASTER
 * on MI355X (119 vs 123-125 us at 4096 x 64: neighbouring rays in flight together hit the same L2 channels), so the
 * shipped binding passes NULL here and hands the order to eslam_render_bwd only, whose scatter needs it.
 * rng_bump (optional): a device counter this launch increments by one (see eslam_sample_z_all_rng).            */
int eslam_render_fwd(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                     const float* rays_o, const float* rays_d, const float* z_vals, int R, int S, float* depth,
                     float* rgb, float* sdf, float* raw_rgb, float* feat, const int32_t* ray_order,
                     uint32_t* rng_bump, eslam_stream_t stream);

/* eslam_render_fwd that also forms the sums of the callers' mapping loss (src/Mapper.py:110-144,337-346) in its
 * epilogue, from the depth / rgb / sdf it holds in registers: acc [ESLAM_LOSS_ACC] and loss [1] (may be NULL) exactly as
 * eslam_loss_value produces them, scratch as there, ray_mask as there (optional).  eslam_loss_grad(acc) then gives the
 * upstream gradients for eslam_render_bwd.  Not for the tracker's loss: its outlier mask depends on the rendered depth. */
int eslam_render_fwd_loss(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                          const float* rays_o, const float* rays_d, const float* z_vals, int R, int S, float* depth,
                          float* rgb, float* sdf, float* raw_rgb, float* feat, const int32_t* ray_order,
                          const float* gt_depth, const float* gt_color, double truncation, const float* weights5_host,
                          const uint8_t* ray_mask, float* scratch, float* acc, float* loss, uint32_t* rng_bump,
                          eslam_stream_t stream);

/* Refresh the half copies of all 12 planes from their float32 masters (both channels-last), one launch: what a
 * mixed-precision training loop runs after every optimiser step.                                            */
int eslam_planes_to_half(const eslam_plane_t* planes, eslam_stream_t stream);

/* Layout change of all 12 planes in one launch, for callers that keep the reference's own NCHW-contiguous planes
 * (src/ESLAM.py:199-210: a texel's 32 channels lie h*w floats apart): field 0 copies src[i].data into the memory
 * dst[i].data points at, field 1 copies src[i].grad into dst[i].grad.  One side of every plane must be dense
 * NCHW-contiguous, the other dense channels-last (stride_c 1, stride_x 32, stride_y 32 w), the same way for all 12.
 * The shipped binding runs it on the planes in front of the kernels and on the gradients behind them whenever the caller's
 * planes are not channels-last and the batch is large enough to pay for 2 x (plane bytes) of HBM traffic; nothing is kept
 * across calls (the mapper swaps the plane Parameters every frame, src/Mapper.py:254-266).                          */
int eslam_planes_relayout(const eslam_plane_t* src, const eslam_plane_t* dst, int field, eslam_stream_t stream);

/* Mixed-precision forward for inference (BASELINE.json configs[4], a tolerance study): planes_f16[i].data points to
 * IEEE-half data of a channels-last [1,32,h,w] plane (strides in half elements: stride_c = 1, stride_x = 32), the decoder
 * weights are rounded to bf16 inside the kernel and run on bf16 MFMA with float32 accumulation; everything after the MLPs
 * (activations, alpha, transmittance, composite) is float32.  Same outputs as eslam_render_fwd.  (Round-1 entry point:
 * the general way is a `data_f16` pointer in every eslam_plane_t, which switches eslam_render_fwd / _fwd_loss / _bwd /
 * _bwd_loss to the mixed-precision kernels, backward included.)                                                   */
int eslam_render_fwd_lowp(const eslam_plane_t* planes_f16, const eslam_decoders_t* dec, const float* bound6_host,
                          const float* rays_o, const float* rays_d, const float* z_vals, int R, int S, float* depth,
                          float* rgb, float* sdf, eslam_stream_t stream);

/* Ray orders for eslam_render_bwd's plane-gradient scatter (and, optionally, eslam_render_fwd): perm, a buffer of
 * ESLAM_RAY_ORDER_WORDS(R) int32 words, <- [ESLAM_RAY_ORDERS][R] permutations followed by 3 floats (+ 1 pad): the angular
 * extent of the batch's fan of rays in each plane, which the scatter reads to choose its workgroup order.  Three
 * permutations of the ray ids, one per plane orientation (xy, xz, yz).  Rays that share one origin (one camera's
 * batch) are sorted, for orientation o, by the azimuth of their direction projected into that plane - the rays of a bundle
 * then cover a thin wedge of the plane and share its cells; batches with several origins get the same order three times
 * (a Morton key of the point one metre along each ray).  Single-pass counting sorts, chunks of 8192 rays.  Depends only on the
 * rays, so a caller can run it on a side stream next to the samplers.  (ABI 5: perm was [R].)                           */
int eslam_ray_order(const float* rays_o, const float* rays_d, int R, int32_t* perm, eslam_stream_t stream);

/* eslam_ray_order and the clear of the iteration's plane-gradient buffer as ONE launch (one node of a captured graph instead
 * of a memset node followed by the order): the ordering workgroups carry the lowest block numbers, the workgroups behind them
 * zero clear_bytes bytes at clear_ptr with 16-byte stores; the two are independent.  clear_ptr must be 16-byte aligned and
 * clear_bytes a multiple of 4, else 1 is returned, eslam_last_error() says why and nothing is launched.  clear_ptr = NULL
 * with clear_bytes = 0 orders only; R = 0 clears only.  (Added under ABI 5.)                                              */
int eslam_ray_order_clear(const float* rays_o, const float* rays_d, int R, int32_t* perm, void* clear_ptr,
                          int64_t clear_bytes, eslam_stream_t stream);

/* The front of a training step as ONE launch on `stream`: what eslam_ray_order_clear (perm, clear_ptr, clear_bytes) and
 * eslam_sample_z_all_rng (everything else) do in two, with the same results - z_vals bit for bit; orders with the same keys
 * (the order inside a key's bin is arbitrary in both).  Nothing is forked to a second stream and nothing has to be joined: the
 * kernels behind it on `stream` find z_vals, perm and the cleared buffer ready.  The argument checks are those of the two
 * entries; 1 is returned, eslam_last_error() says why and nothing is launched when one fails.  perm = NULL with
 * clear_bytes = 0 is eslam_sample_z_all_rng; R = 0 clears only.  (Added under ABI 5.)                                       */
int eslam_step_front(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                     const float* rays_o, const float* rays_d, const float* gt_depth, int R, int n_strat, int n_imp,
                     double truncation, const float* t_free, const float* t_surf, int perturb, uint64_t seed,
                     const uint32_t* rng_state, int64_t ray_offset, float* z_vals, int32_t* perm, void* clear_ptr,
                     int64_t clear_bytes, eslam_stream_t stream);

/* Bytes of scratch eslam_render_bwd / eslam_decode_bwd need for n_points = R*S points.               */
int64_t eslam_bwd_workspace_bytes(int64_t n_points);

/* K8 backward of eslam_render_fwd (autograd of the lines above).
 * Upstream: g_depth [R], g_rgb [R,3], g_sdf [R,S] (any may be NULL = zero).
 * Accumulates into planes[i].grad (where non-NULL), OVERWRITES g_dec [ESLAM_N_DEC_PARAMS] (order of
 * eslam_decoders_t: w1,b1,w2,b2,w3,b3,cw1,...,cb3; NULL = decoders frozen, their gradient work is skipped) and
 * g_beta [1] (may be NULL), and when g_rays_o / g_rays_d are
 * non-NULL overwrites them ([R,3] each) with the gradient through pts = o + d z.  z_vals carries no gradient
 * (Renderer.py builds it under no_grad / from gt_depth).  ray_order: the buffer eslam_ray_order filled, or NULL
 * (then the order is computed here).
 * Mixed precision (planes with data_f16): the same outputs, g_rays_o / g_rays_d included - the position gradient is taken
 * on the half copies, behind the scatter, or behind the decoder backward alone when no plane takes a gradient (tracking).
 * workspace: eslam_bwd_workspace_bytes(R*S) bytes.                                                          */
int eslam_render_bwd(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                     const float* rays_o, const float* rays_d, const float* z_vals, int R, int S,
                     const float* sdf, const float* raw_rgb, const float* feat, const float* g_depth,
                     const float* g_rgb, const float* g_sdf, float* g_dec, float* g_beta, float* g_rays_o,
                     float* g_rays_d, const int32_t* ray_order, void* workspace, eslam_stream_t stream);

/* eslam_render_bwd for an iteration whose loss is the mapping loss (src/Mapper.py:110-144,337-346; with ray_mask the
 * tracker's, src/Tracker.py:114-148,197-204): the upstream gradients d loss / d (depth, rgb, sdf) are formed INSIDE the
 * backward kernel from acc [ESLAM_LOSS_ACC] - the set sizes and sums eslam_render_fwd_loss / eslam_loss_value /
 * eslam_loss_reduce (+ all-reduce) produced - instead of being written by eslam_loss_grad and read back: loss gradient,
 * composite backward and decoder backward are one launch.  depth [R], rgb [R,3]: the forward outputs.  upstream [1] on
 * the device = d L / d loss (NULL = 1).  loss_out [1] (optional): receives the loss value formed from acc (a ray-sharded
 * caller's acc is only complete after its all-reduce).  g_depth / g_rgb / g_sdf (each optional): FURTHER upstream
 * gradients on the rendered outputs, added to the loss's own.  Everything else as eslam_render_bwd, the ray gradients
 * of the mixed-precision path included.
 * Both entries: a ray whose upstream gradients are all exactly zero - one that ray_mask, or the mask of eslam_loss_grad,
 * takes out of the batch - contributes exactly 0.0 to every gradient, and its own g_rays_o / g_rays_d rows are 0.0,
 * whatever its z_vals hold (the NaN row of a ray whose AABB exit is 0/0 included): zeros are selected, not multiplied. */
int eslam_render_bwd_loss(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                          const float* rays_o, const float* rays_d, const float* z_vals, int R, int S,
                          const float* sdf, const float* raw_rgb, const float* feat, const float* depth,
                          const float* rgb, const float* gt_depth, const float* gt_color, double truncation,
                          const float* weights5_host, const uint8_t* ray_mask, const float* acc,
                          const float* upstream, float* loss_out, const float* g_depth, const float* g_rgb,
                          const float* g_sdf, float* g_dec, float* g_beta, float* g_rays_o, float* g_rays_d,
                          const int32_t* ray_order, void* workspace, eslam_stream_t stream);

/* The saved first hidden layer (float32 planes).  The four entries above with one more pointer in front of `stream`:
 * hidden, eslam_saved_hidden_floats(R, S) = 2 * R * ceil(S / 16) * 256 floats (128 bytes per sample when S is a multiple
 * of 16), or NULL.  The forward entries fill it with h1 = relu(W1 . feat + b1) of both decoders as their kernel holds it - block
 * (decoder d, ray, sb = 16 samples) at float offset ((d * R + ray) * ceil(S / 16) + sb) * 256, unit 4q + i of point r of the block
 * at (16 q + r) * 4 + i, blocks stored whole - and need feat with it; R * ceil(S / 16) * 2048 < 2^32 - 256 (32-bit byte
 * offsets), else an error.  The backward entries, given the buffer the forward pass of the same call filled, read h1 from it
 * instead of recomputing it from feat (16 of a block's 52 MFMAs): every output has the same bits.  NULL: the entries above,
 * which are these with NULL.  Planes with data_f16 (mixed precision) ignore the pointer.                                   */
int64_t eslam_saved_hidden_floats(int64_t R, int S);
int eslam_render_fwd_h(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                       const float* rays_o, const float* rays_d, const float* z_vals, int R, int S, float* depth,
                       float* rgb, float* sdf, float* raw_rgb, float* feat, const int32_t* ray_order,
                       uint32_t* rng_bump, float* hidden, eslam_stream_t stream);
int eslam_render_fwd_loss_h(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                            const float* rays_o, const float* rays_d, const float* z_vals, int R, int S, float* depth,
                            float* rgb, float* sdf, float* raw_rgb, float* feat, const int32_t* ray_order,
                            const float* gt_depth, const float* gt_color, double truncation, const float* weights5_host,
                            const uint8_t* ray_mask, float* scratch, float* acc, float* loss, uint32_t* rng_bump,
                            float* hidden, eslam_stream_t stream);
int eslam_render_bwd_h(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                       const float* rays_o, const float* rays_d, const float* z_vals, int R, int S,
                       const float* sdf, const float* raw_rgb, const float* feat, const float* g_depth,
                       const float* g_rgb, const float* g_sdf, float* g_dec, float* g_beta, float* g_rays_o,
                       float* g_rays_d, const int32_t* ray_order, void* workspace, const float* hidden,
                       eslam_stream_t stream);
int eslam_render_bwd_loss_h(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                            const float* rays_o, const float* rays_d, const float* z_vals, int R, int S,
                            const float* sdf, const float* raw_rgb, const float* feat, const float* depth,
                            const float* rgb, const float* gt_depth, const float* gt_color, double truncation,
                            const float* weights5_host, const uint8_t* ray_mask, const float* acc,
                            const float* upstream, float* loss_out, const float* g_depth, const float* g_rgb,
                            const float* g_sdf, float* g_dec, float* g_beta, float* g_rays_o, float* g_rays_d,
                            const int32_t* ray_order, void* workspace, const float* hidden, eslam_stream_t stream);

/* Decoder-only query.  Replaces src/networks/decoders.py:127-146 (Decoders.forward), the entry used by
 * src/utils/Mesher.py:151 on up to 500k points.  pts [N,3] world coordinates -> raw [N,4] = (r,g,b,sdf).
 * flags: ESLAM_DECODE_SDF_ONLY evaluates geometry planes + SDF decoder only (decoders.py:87-105) and writes
 * raw [N,1]; ESLAM_DECODE_MASK_OUTSIDE sets the sdf of every point that is not strictly inside the bound to -1
 * (Mesher.eval_points, src/utils/Mesher.py:146-153).  feat [N,128] optional (needed only for eslam_decode_bwd). */
#define ESLAM_DECODE_SDF_ONLY 1
#define ESLAM_DECODE_MASK_OUTSIDE 2
int eslam_decode_fwd(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                     const float* pts, int64_t N, int flags, float* raw, float* feat, eslam_stream_t stream);

/* The SDF and its gradient with respect to the point, fused: pts [N,3] world coordinates -> sdf [N] (may be NULL) and
 * grad [N,3] = d sdf / d p.  The reference has no equivalent (its only route is autograd through Decoders.forward).
 * sdf is what eslam_decode_fwd(ESLAM_DECODE_SDF_ONLY) writes for the same points, bit for bit (the same tile, the same
 * operation order, no outside mask).  grad is what autograd of that sdf gives: per world axis a factor 2 / (hi - lo)
 * (normalize_3d_coordinate, src/common.py:215-217); per plane axis of n texels a factor (n - 1) / 2, and 0 where the border
 * clamp is active (the coordinate on or outside the bound: ATen's clip_coordinates_set_grad), so such a component is
 * exactly 0; a ReLU's derivative is 1 where its pre-activation is > 0, else 0; a last factor 1 - sdf^2 from the tanh.
 * flags: ESLAM_SDF_GRAD_UNIT divides every row by sqrtf(grad . grad) and writes (0, 0, 0) where grad . grad == 0.
 * Only planes[0..5] (geometry, both levels) and the SDF decoder (w1 .. b3) are read.  Planes channels-last or the
 * reference's NCHW, float32 only: with half copies present (data_f16) the float32 masters are read.
 * One launch on `stream`, never synchronises, nothing per point in device memory but pts, sdf and grad; a grid of at most
 * ESLAM_SDF_GRAD_MAX_GROUPS workgroups of 256 points walks the tiles.  N = 0 is valid and launches nothing; bad arguments
 * (N < 0, unknown flags, a null pointer, a bad plane) come back non-zero, with eslam_last_error() set, before any launch. */
#define ESLAM_SDF_GRAD_UNIT 1
#define ESLAM_SDF_GRAD_MAX_GROUPS 8192
int eslam_sdf_grad(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                   const float* pts, int64_t N, int flags, float* sdf, float* grad, eslam_stream_t stream);

/* The SDF of an implicit grid: eslam_decode_fwd(ESLAM_DECODE_SDF_ONLY | flags) on the points (xs[ix], ys[iy], zs[iz]),
 * which are never materialised.  Replaces the field half of src/utils/Mesher.py:196-217 (get_grid_uniform's points,
 * Mesher.py:178-184, through eval_points in 500k batches, then z[~mask] = -1 with the frame hull's mask).
 * xs [nx], ys [ny], zs [nz]: ascending float32 axes (np.linspace cast to float32, Mesher.py:170-180).
 * vol [nx][ny][nz] (z fastest) = the reference's z.reshape(ny, nx, nz).transpose(1, 0, 2) (Mesher.py:224-226).
 * halfspaces [n_halfspaces] float4 (nx, ny, nz, d), 16-byte aligned, may be NULL when n_halfspaces = 0: a point is inside
 * the region when n.p + d <= 0 for all of them; vol is -1 outside the region.  flags: ESLAM_DECODE_MASK_OUTSIDE as for
 * eslam_decode_fwd (-1 where the point is not strictly inside bound6); ESLAM_DECODE_SDF_ONLY is implied.
 * Runs of 64 points along z are culled as segments: entirely outside the bound or one half-space -> -1 without a
 * decode; both ends inside every half-space -> no per-point test.                                              */
int eslam_sdf_grid(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                   const float* xs, const float* ys, const float* zs, int64_t nx, int64_t ny, int64_t nz,
                   const float* halfspaces, int n_halfspaces, int flags, float* vol, eslam_stream_t stream);

/* Marching cubes on vol [nx][ny][nz] (z fastest) at `level`.  Replaces skimage.measure.marching_cubes in
 * src/utils/Mesher.py:222-239 (without Lewiner's interior-ambiguity resolution; tables: eslam_mc_tables.h).
 * Two phases, one host sync in between:
 *   eslam_mc_count  writes counts [2] (device int64) = (n_verts, n_faces); the caller reads them and allocates
 *   eslam_mc_emit   fills verts [n_verts,3] float32 and faces [n_faces,3] int32; same vol, level and workspace.
 * workspace: eslam_mc_workspace_bytes(nx, ny, nz) bytes (6 per grid point + 16 per 4096), kept between the calls.
 * Output contract:
 *   one vertex per crossing edge (one end < level, the other not) along +x, +y or +z from a grid point, shared by
 *   every cube around it, ordered by that point's linear index, then axis x, y, z;  position
 *   origin + (i + t) * spacing along the edge's axis, t = (level - v_lo) / (v_hi - v_lo), v_lo at the lower index
 *   (origin, spacing float64 as Mesher.py:228-230,246);
 *   faces ordered by cube (= its lower corner's linear index), then table order; (v1 - v0) x (v2 - v0) points toward
 *   values >= level.  More than 2^31 - 1 vertices is an error of eslam_mc_emit.                                 */
int64_t eslam_mc_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);
int eslam_mc_count(const float* vol, int64_t nx, int64_t ny, int64_t nz, float level, void* workspace, int64_t* counts,
                   eslam_stream_t stream);
int eslam_mc_emit(const float* vol, int64_t nx, int64_t ny, int64_t nz, float level, const double* origin3_host,
                  const double* spacing3_host, const void* workspace, int64_t n_verts, int64_t n_faces, float* verts,
                  int32_t* faces, eslam_stream_t stream);

/* eslam_mc_count for a volume of which only part was observed: weight [nx][ny][nz] float32, a grid point is valid when
 * its weight > 0.  A cube keeps its faces only when all eight corners are valid; an edge keeps its vertex only when it
 * crosses the level and at least one of the (up to four) cubes around it is fully valid, so no vertex is left without a
 * face.  Order, orientation, positions and the workspace are those of eslam_mc_count; eslam_mc_emit follows, unchanged
 * (it reads the workspace).  With every weight > 0 (and nx, ny, nz >= 2, so that every edge has a cube) the result equals
 * eslam_mc_count's bit for bit.                                                                                  */
int eslam_mc_count_masked(const float* vol, const float* weight, int64_t nx, int64_t ny, int64_t nz, float level,
                          void* workspace, int64_t* counts, eslam_stream_t stream);

/* TSDF fusion of n_frames depth (and colour) images into a dense volume over a box: replaces the integrate step of
 * open3d's ScalableTSDFVolume in src/utils/Mesher.py:63-128.  tsdf, weight [nx][ny][nz] float32 (z fastest; weight = the
 * number of observations), color [nx][ny][nz][3] float32 or NULL; voxel (i, j, k) has its centre at
 * origin + (index + 0.5) voxel.  depths [n_frames][H][W], colors [n_frames][H][W][3] (NULL iff color is NULL),
 * w2c [n_frames][12] (device): the 3x4 rows (float32) of the float64 inverse, taken on the host, of c2w with its columns 1
 * and 2 negated (Mesher.py:94-96: the camera looks along +z, x right, y down); depth_max [n_frames] (device): an upper
 * bound of each frame's depth, used only to skip work (NaN or inf: nothing is skipped).
 * Per voxel, frames in index order k = 0 .. n_frames - 1, every operation float32, left to right, not contracted:
 *   p    = origin + (float(i) + 0.5f) * voxel                         (per axis)
 *   c    = w2c[k] [p, 1]                                              ((r0 px + r1 py) + r2 pz) + t  per row
 *   skip unless c.z > 0
 *   u    = (fx c.x) / c.z + cx;   v = (fy c.y) / c.z + cy
 *   iu   = floor(u + 0.5f);       iv = floor(v + 0.5f)                skip unless 0 <= iu < W and 0 <= iv < H
 *   d    = depths[k][iv][iu]                                          skip unless d > 0 (NaN skips)
 *   xn   = (float(iu) - cx) / fx; yn = (float(iv) - cy) / fy
 *   m    = sqrtf((1 + xn xn) + yn yn)                                 ray length per unit z
 *   sdf  = (d - c.z) m                                                skip unless sdf > -trunc
 *   t    = fminf(1, sdf / trunc); W1 = weight + 1
 *   tsdf = (tsdf weight + t) / W1;  color likewise per channel from colors[k][iv][iu];  weight = W1
 * The projective running average of open3d's integrate: nearest pixel, distance along the ray.  No weight cap.
 * Calls compose: frames 0 .. a in one call and a + 1 .. b in the next give the bits of one call with 0 .. b.
 * A run of 64 voxels along z that no frame of the call updates is neither read nor written.  H, W <= 16384.        */
int eslam_tsdf_integrate(float* tsdf, float* weight, float* color, int64_t nx, int64_t ny, int64_t nz,
                         const float* origin3_host, float voxel, float trunc, const float* depths, const float* colors,
                         const float* w2c, const float* depth_max, int n_frames, int H, int W, float fx, float fy, float cx,
                         float cy, eslam_stream_t stream);

/* out [n,3] = color [nx][ny][nz][3] sampled trilinearly at pts [n,3] (world coordinates, float32): per axis
 * g = (p - origin) / voxel - 0.5 (voxel-centre coordinates), i0 = floor(g), t = g - i0, the indices i0 and i0 + 1 clamped
 * to the volume.  On a marching-cubes vertex of the volume this is the linear blend of the edge's two voxels.      */
int eslam_tsdf_sample_color(const float* color, int64_t nx, int64_t ny, int64_t nz, const float* origin3_host, float voxel,
                            const float* pts, int64_t n, float* out, eslam_stream_t stream);

/* Frame preparation: the decoded images of one RGB-D frame -> the float32 images the loop samples; replaces the host
 * arithmetic of src/utils/datasets.py:88-114 (BaseDataset.__getitem__).  rgb [Hc][Wc][3] uint8 (RGB), depth [Hd][Wd] uint16,
 * both on the device.  Stages, each absent when it is the identity:
 *   1  colour resized to (Hd, Wd): bilinear on pixel centres (cv2.resize; F.interpolate align_corners=False)
 *   2  both resized to crop_size (crop_h, crop_w; 0, 0 = none): colour bilinear with aligned corners, depth nearest with
 *      torch's float32 rule  src = min(int(floorf(dst * (float(in) / float(out)))), in - 1)
 *   3  crop_edge pixels dropped on every side
 *   4  colour / 255;  depth = (float(raw) / png_depth_scale) * scale, two float32 operations, the division a true one
 * color_out [H'][W'][3], depth_out [H'][W'] float32 with (H', W') = eslam_frame_out_shape(...).  The colour stages are
 * evaluated per output pixel by nested taps (no intermediate image); tap positions and weights follow torch's upsample
 * arithmetic in float64 (src = in/out (dst + 0.5) - 0.5 clamped at 0, or (in-1)/(out-1) dst with aligned corners;
 * i0 = int(src), i1 = i0 + (i0 < in - 1), w1 = src - i0, w0 = 1 - w1), are rounded to float32, and the blends
 * wy0 (wx0 a + wx1 b) + wy1 (wx0 c + wx1 d) are float32 on byte values, the division by 255 last.  With no stage at all
 * (and 16-byte aligned outputs) one flat launch converts both images four elements per lane.  Sizes <= 16384.        */
int eslam_frame_out_shape(int Hc, int Wc, int Hd, int Wd, int crop_h, int crop_w, int crop_edge, int* H_out_host,
                          int* W_out_host);
int eslam_frame_prepare(const uint8_t* rgb, int Hc, int Wc, const uint16_t* depth, int Hd, int Wd, int crop_h, int crop_w,
                        int crop_edge, float png_depth_scale, float scale, float* color_out, float* depth_out,
                        eslam_stream_t stream);

/* Lens undistortion of a byte image (TUM RGB-D; cv2.undistort restated as F.grid_sample(bilinear, zeros,
 * align_corners=True) in datasets.undistort): out [H][W][3] uint8 = rgb sampled at grid [H][W][2] (float32, x then y in
 * [-1, 1] coordinates; datasets.undistort_map), float32 in the order of torch's CPU kernel: pixel = (g + 1) ((size - 1) / 2),
 * fractions w, n and e = 1 - w, s = 1 - n, value = fma(se, w n, fma(sw, e n, fma(ne, w s, nw (e s)))) with taps outside
 * the image 0, then round-half-even and clamp to [0, 255].  out must not be rgb.                                      */
int eslam_frame_undistort(const uint8_t* rgb, const float* grid, int H, int W, uint8_t* out, eslam_stream_t stream);

/* Mesh culling: the visibility test of src/tools/cull_mesh.py:61-104 for a chunk of n_frames frames in one launch.
 * For every vertex p of verts [n_verts,3] whose seen[p] is 0 and every frame k, with w2c[k] the 3x4 rows (float32,
 * inverted from c2w on the host in float64) of w2c [n_frames][12] (device):
 *   c = w2c[k] [p, 1];  a = fx (-c.x) + cx c.z;  b = fy c.y + cy c.z;  zz = c.z + 1e-5;  u = a / zz;  v = b / zz;
 *   seen when -zz >= 0, 0 < u < W and 0 < v < H, and with depth_test (cfg['meshing']['eval_rec']) also
 *   d + truncation >= -zz, d = the bilinear, zero-padded sample of depths[k] ([n_frames][depth_h][depth_w]) at pixel
 *   (u (depth_w - 1) / W, v (depth_h - 1) / H) (grid_sample, align_corners=True, of the grid 2 (u / W, v / H) - 1).
 * seen [n_verts] uint8 is ORed into (set to 1, never cleared).  depths may be NULL when depth_test is 0.            */
int eslam_cull_vertices(const float* verts, int64_t n_verts, const float* depths, int n_frames, int depth_h, int depth_w,
                        const float* w2c, float fx, float fy, float cx, float cy, int H, int W, float truncation,
                        int depth_test, uint8_t* seen, eslam_stream_t stream);

/* Exact nearest neighbours on a uniform grid of cubic cells: replaces scipy's cKDTree.query in
 * src/tools/eval_recon.py:21-39 and open3d's correspondence search of registration_icp (eval_recon.py:42-56).
 * Grid rule (eslam_nn_grid_plan, from the point count N and the bounding box [lo, hi] of the reference points):
 *   E = the largest extent; E = 0 (one point, or all equal): one cell of edge 1.  Otherwise the m axes with extent
 *   > 1e-6 E span the volume P (product of their extents), the target cell count is C = min(MAX_CELLS,
 *   CELLS_PER_POINT * N), the edge h = (P / C)^(1/m), and dims[d] = max(1, ceil(extent[d] / h)) (flat axes: 1 cell).
 *   While dims[0] dims[1] dims[2] > MAX_CELLS, h grows by 10 %.  The stored edge is the float32 just above h.
 * Build: a counting sort of the reference points into cell order, kept in the workspace as float4 (x, y, z, index).
 * Query: dist [n_query] = sqrt of the float32 squared distance to the nearest reference point, idx [n_query] its index;
 *   equal distances go to the smaller index, so results are bit-identical run to run.  Exact for every query,
 *   including ones far outside the box.  max_dist finite: only points with dist < max_dist count, none -> (inf, -1);
 *   INFINITY = no limit.  flags: ESLAM_NN_INPUT_ORDER = process the queries in input order (no query workspace,
 *   query_workspace may be NULL); by default they are first sorted by cell, the same counting sort.
 * Workspaces: eslam_nn_workspace_bytes (kept between the build and every query), eslam_nn_query_workspace_bytes.      */
#define ESLAM_NN_MAX_CELLS (1 << 24)
#define ESLAM_NN_CELLS_PER_POINT 2
#define ESLAM_NN_INPUT_ORDER 1
typedef struct {
    float lo[3];       /* the reference points' minimum corner */
    float cell;        /* edge of the cubic cells             */
    int32_t dims[3];   /* cells per axis                      */
    int32_t reserved;
} eslam_nn_grid_t;
int eslam_nn_grid_plan(int64_t n_ref, const float* bbox6_host, eslam_nn_grid_t* grid);
int64_t eslam_nn_workspace_bytes(const eslam_nn_grid_t* grid, int64_t n_ref);
int eslam_nn_build(const float* ref, int64_t n_ref, const eslam_nn_grid_t* grid, void* workspace, eslam_stream_t stream);
int64_t eslam_nn_query_workspace_bytes(const eslam_nn_grid_t* grid, int64_t n_query);
int eslam_nn_query(const eslam_nn_grid_t* grid, const void* workspace, int64_t n_ref, const float* queries,
                   int64_t n_query, float max_dist, int flags, void* query_workspace, float* dist, int32_t* idx,
                   eslam_stream_t stream);

/* The moments of one point-to-point ICP round (open3d's TransformationEstimationPointToPoint, eval_recon.py:52-54) over
 * the correspondences i with idx[i] >= 0 and dist[i] < threshold, s = src[i], t = tgt[idx[i]]:
 * out [17] (device, float64) = count, sum d^2, sum s (3), sum t (3), sum s t^T (9, row-major).  A fixed-order tree
 * (no float atomics): bit-identical run to run.  workspace: eslam_icp_moments_workspace_bytes() bytes.           */
int64_t eslam_icp_moments_workspace_bytes(void);
int eslam_icp_moments(const float* src, const float* tgt, const float* dist, const int32_t* idx, int64_t n,
                      float threshold, void* workspace, double* out, eslam_stream_t stream);

/* Exact point-to-mesh distance on a uniform grid of cubic cells (no counterpart in the reference, whose 3D metrics
 * measure to a sample cloud).  verts [n_verts,3] float32, faces [n_faces,3] int32, queries [n_query,3] float32, device.
 * Grid rule (eslam_tri_grid_plan, host only; bbox6 = lo/hi per axis of the finite vertices, face_extent = the mean
 * over the faces of the largest axis extent of the face's box, as the caller measured it):
 *   E = the largest extent of the box; E = 0 or n_faces = 0: one cell of edge 1.  Otherwise the m axes with extent
 *   > 1e-6 E span the volume P; the edge is h = max(ESLAM_TRI_CELL_PER_EXTENT * face_extent, (P / MAX_CELLS)^(1/m)),
 *   with (P / n_faces)^(1/m) in place of the first term when face_extent is not positive and finite;
 *   dims[d] = max(1, ceil(extent[d] / h)); while their product > MAX_CELLS, h grows by 10 %.  The stored edge is the
 *   float32 just above h.  A cell of two face extents holds a face in about two cells.
 * Entries: a face is entered in every cell its axis-aligned box overlaps; a face with a non-finite coordinate or an
 *   index outside [0, n_verts) is entered nowhere and is never returned.  eslam_tri_count writes total [2] (device,
 *   int64) = the number of (face, cell) entries and of faces entered; the caller copies total[0] into grid->entries.
 *   eslam_tri_workspace_bytes and eslam_tri_build fail, before any launch and naming the count, when grid->entries
 *   is negative or above ESLAM_TRI_MAX_ENTRIES (2^31 - 1).  The workspace keeps, in cell order, three float4 per entry:
 *   (a, face index bits), (b, 0), (c, 0).
 * Query: one query per lane, rings of growing Chebyshev radius round the query's clamped cell; it stops when the face
 *   distance of the searched box, less a slack of 4e-6 (|q|_inf + |box|_inf), squared, reaches the best so far.
 *   The result is the minimum over ALL entered faces of the per-pair function below, (d2, face) lexicographically:
 *   equal d2 go to the smaller face index.  dist [n_query] = sqrtf(d2), face [n_query], closest [n_query,3] (may be
 *   NULL).  max_dist as for eslam_nn_query: only dist < max_dist counts.  A query with a non-finite coordinate, or
 *   with no face in reach, gets dist = inf, face = -1, closest = NaN.  n_query = 0 or grid->entries = 0 returns 0
 *   without a launch and writes nothing: with no entries the caller fills (inf, -1).
 *   flags: ESLAM_TRI_INPUT_ORDER = queries in input order (no query workspace); by default in cell order.
 * The per-pair function (Ericson's closest point on a triangle), float32 operation by operation, no contraction;
 * dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z;  ab = b - a,  ac = c - a  (a vertex region returns the vertex itself):
 *   ap = q - a;  d1 = dot(ab, ap);  d2 = dot(ac, ap);          d1 <= 0 and d2 <= 0                 -> a
 *   bp = ap - ab;  d3 = dot(ab, bp);  d4 = dot(ac, bp);        d3 >= 0 and d4 <= d3                -> b     
 *   vc = d1 d4 - d3 d2;   vc <= 0, d1 >= 0, d3 <= 0:           s = d1 - d3,  v = d1 / s            -> a + ab v
 *   cp = ap - ac;  d5 = dot(ab, cp);  d6 = dot(ac, cp);        d6 >= 0 and d5 <= d6                -> c     
 *   vb = d5 d2 - d1 d6;   vb <= 0, d2 >= 0, d6 <= 0:           s = d2 - d6,  w = d2 / s            -> a + ac w
 *   va = d3 d6 - d5 d4;   va <= 0, d4 - d3 >= 0, d5 - d6 >= 0: s = (d4 - d3) + (d5 - d6), w = (d4 - d3) / s
 *                                                                                       -> b + (c - b) w
 *   otherwise s = (va + vb) + vc,  r = 1 / s,  v = vb r,  w = vc r                      -> (a + ab v) + ac w
 *   (the tests in this order, the first that holds decides; u t = per component product, then the sum).
 *   The interior branch also requires va, vb and vc each above tol = (1e-6 (n1(ab) n1(ac))) (m m), with
 *   n1(u) = (|u.x| + |u.y|) + |u.z| and m = (n1(ap) + n1(ab)) + n1(ac): a bound on the rounding noise of these
 *   differences of products, below which (collinear and sliver faces) the weights v, w would be arbitrary.
 *   When the deciding branch has an s that is not positive and finite, or the interior is not clear of tol (zero-area
 *   and sliver faces, projections within about 1e-4 of a face's size of an edge, overflow), the
 *   closest point is the nearest of the three segments (a, ab), (a, ac), (b, c - b), the first of equal ones:
 *   on (o, e): ee = dot(e, e), t = min(max(dot(q - o, e) / ee, 0), 1) when ee is positive and finite, else 0 (a NaN
 *   quotient gives 0); point o + e t.
 *   Then d = q - closest, d2 = (d.x d.x + d.y d.y) + d.z d.z.  A pair whose d2 is NaN (overflow: coordinates beyond
 *   about 1e8) is never selected, so no output is ever NaN.                                                         */
#define ESLAM_TRI_MAX_CELLS (1 << 24)
#define ESLAM_TRI_CELL_PER_EXTENT 2
#define ESLAM_TRI_MAX_ENTRIES 2147483647LL
#define ESLAM_TRI_INPUT_ORDER 1
typedef struct {
    float lo[3];       /* the vertices' minimum corner                              */
    float cell;        /* edge of the cubic cells                                   */
    int32_t dims[3];   /* cells per axis                                            */
    int32_t reserved;
    int64_t entries;   /* (face, cell) entries: 0 from the plan, then eslam_tri_count's */
} eslam_tri_grid_t;
int eslam_tri_grid_plan(int64_t n_faces, const float* bbox6_host, float face_extent, eslam_tri_grid_t* grid);
int eslam_tri_count(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                    const eslam_tri_grid_t* grid, int64_t* total, eslam_stream_t stream);
int64_t eslam_tri_workspace_bytes(const eslam_tri_grid_t* grid);
int eslam_tri_build(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                    const eslam_tri_grid_t* grid, void* workspace, eslam_stream_t stream);
int64_t eslam_tri_query_workspace_bytes(const eslam_tri_grid_t* grid, int64_t n_query);
int eslam_tri_query(const eslam_tri_grid_t* grid, const void* workspace, const float* queries, int64_t n_query,
                    float max_dist, int flags, void* query_workspace, float* dist, int32_t* face, float* closest,
                    eslam_stream_t stream);

/* Mesh clean-up (src/tools/clean_mesh.py): the vertex merge of trimesh's process() that closes the reference's
 * src/tools/cull_mesh.py:109, and the connected components behind NICE-SLAM's remove_small_geometry.  verts [n_verts,3]
 * float32, faces [n_faces,3] int32 with every index in [0, n_verts) (the caller checks: the kernels do not).  Counts are
 * 0 .. ESLAM_MESH_MAX_COUNT; a count outside comes back non-zero before any launch, zero vertices return 0 without one.
 * Every result is a function of the input alone (a smallest index, an exact integer sum): bit-identical run to run.
 *
 * eslam_mesh_weld: rep [n_verts] int32 = the smallest index u whose position equals v's, coordinate by coordinate as
 *   floats with -0 == +0 (bit patterns compared after -0 is turned into +0: one ulp apart is different, denormals are
 *   ordinary values); a vertex with a NaN or infinite coordinate gets -1 and takes no part.
 *   workspace: eslam_mesh_weld_workspace_bytes(n_verts) bytes, any contents: an open-addressing table of int32 vertex
 *   indices with S slots, S the power of two >= 2 n_verts and >= ESLAM_MESH_WELD_MIN_SLOTS; 4 S bytes (-1 for a bad count).
 * eslam_mesh_components: label [n_verts] int32 = the smallest vertex index of v's component, where two vertices are
 *   connected when a chain of faces that share a VERTEX joins them (trimesh splits by shared EDGES: two pieces touching at
 *   one vertex are one component here).  A vertex in no face labels itself; a face may repeat an index.
 * eslam_mesh_component_sizes: face_count [n_verts] int32, cleared by the call, then face_count[label[faces[f][0]]] += 1
 *   for every face: the face count of a component at its label, 0 elsewhere.  Integer atomics: exact.                 */
#define ESLAM_MESH_MAX_COUNT (1 << 30)
#define ESLAM_MESH_WELD_MIN_SLOTS 64
int64_t eslam_mesh_weld_workspace_bytes(int64_t n_verts);
int eslam_mesh_weld(const float* verts, int64_t n_verts, void* workspace, int32_t* rep, eslam_stream_t stream);
int eslam_mesh_components(const int32_t* faces, int64_t n_faces, int64_t n_verts, int32_t* label, eslam_stream_t stream);
int eslam_mesh_component_sizes(const int32_t* faces, int64_t n_faces, const int32_t* label, int64_t n_verts,
                               int32_t* face_count, eslam_stream_t stream);

/* Depth images of a triangle mesh for a chunk of n_views views in one call: replaces open3d's visualiser in
 * src/tools/eval_recon.py:177-201 (capture_depth_float_buffer(True) with mesh_show_back_face and set_constant_z_far(20)).
 * verts [n_verts,3] float32, faces [n_faces,3] int32, w2c [n_views][12] the 3x4 rows (float32, inverted from c2w on the
 * host in float64) of the reference's param.extrinsic = inv(c2w): the camera looks along +z, x right, y down.
 * depth [n_views][H][W] float32 = the camera-space z of the nearest surface at each pixel centre, 0 where nothing is hit.
 * Per view, with v0, v1, v2 a triangle's vertices in the camera frame (v = w2c [p, 1], float32) and
 * d = ((i - cx) / fx, (j - cy) / fy, 1) the ray of pixel (column i, row j):
 *   edge functions  E0 = d . (v1 x v2),  E1 = d . (v2 x v0),  E2 = d . (v0 x v1), each cross product evaluated from
 *                   the edge's smaller end (camera-space x, then y, then z) as lo x (hi - lo), negated when that end is
 *                   v_j: the same value without the cancellation of two long vectors, and the same bits up to the sign
 *                   in the two triangles that share the edge;
 *   covered         when E0, E1, E2 >= 0 or E0, E1, E2 <= 0: no back-face culling, and zero counts as inside, so a
 *                   shared edge leaves no hole;
 *   depth           z = (n . v0) / (n . d),  n = (v1 - v0) x (v2 - v0);  n . d = 0 (ray in the plane) is no hit;
 *   a hit counts    when z_near <= z <= z_far; the pixel keeps the smallest such z over all triangles.
 * There is no perspective divide of vertices and so no near-plane clipping: a triangle that straddles the camera plane
 * renders its part beyond z_near.  Skipped: a triangle with n = 0, one whose largest vertex z is below z_near or whose
 * smallest is above z_far, one with a vertex index outside [0, n_verts).  Pixel box: the projections' bounds widened by
 * 0.01 px, clamped to the image; with a vertex at z <= z_near, the bounds of the triangle's part beyond z_near / 2 (the
 * polygon cut by that plane, its corners projected) widened by 1 px.
 * The z-buffer is the output itself, as uint32 holding the float's bits (positive floats order as their bit patterns):
 * cleared to 0x7f800000, resolved with atomicMin, untouched pixels turned into 0 by a last pass - all inside the call.
 * min is order-independent: two calls give bit-identical images, and a chunk equals its views rendered one by one.
 * large_area: a triangle whose pixel box holds more than large_area pixels is cut into 64 x 64 pixel tiles, queued and
 * rasterised a wave per tile; a smaller one is rasterised by the lane that set it up.  <= 0 = ESLAM_RASTER_LARGE_AREA.
 * The images do not depend on it.  workspace: eslam_raster_workspace_bytes(n_faces, n_views, H, W) bytes, any contents
 * (a counter and a queue of at most 2^19 tiles per view; tiles beyond the queue are rasterised by their triangle's lane).
 * H, W <= 16384.  Deviation: z_near is the caller's constant (ESLAM_RASTER_Z_NEAR in our metric); open3d derives its
 * near plane from the scene's bounding box.                                                                        */
#define ESLAM_RASTER_LARGE_AREA 64
#define ESLAM_RASTER_Z_NEAR 0.01f
#define ESLAM_RASTER_Z_FAR 20.0f
int64_t eslam_raster_workspace_bytes(int64_t n_faces, int n_views, int H, int W);
int eslam_raster_depth(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* w2c,
                       int n_views, float fx, float fy, float cx, float cy, int H, int W, float z_near, float z_far,
                       int large_area, void* workspace, float* depth, eslam_stream_t stream);

/* out [n_views] (device, float64) = per view the sum over its n_pixels pixels of |a - b|, a and b [n_views][n_pixels]
 * float32 (np.abs(gt_depth - ours_depth) of eval_recon.py:203 before the mean; empty pixels are 0 in both images and
 * take part).  A fixed-order tree in float64 (no float atomics): bit-identical run to run.
 * workspace: eslam_depth_l1_workspace_bytes(n_views) bytes.  n_views <= 65535.                                       */
int64_t eslam_depth_l1_workspace_bytes(int n_views);
int eslam_depth_l1(const float* a, const float* b, int n_views, int64_t n_pixels, void* workspace, double* out,
                   eslam_stream_t stream);

/* The offline viewer's headless colour renderer (reference src/tools/visualizer_util.py:178-200: the open3d window with
 * point_size = 4 and mesh_show_back_face = False, showing an unlit mesh and point clouds).  All geometry of a chunk of
 * views composes through one buffer of uint64 keys [n_views][H][W] at the start of `workspace`: the high word is the bits
 * of the camera-space depth z (a positive float orders as its bits), the low word the pixel's RGBA8, R in the lowest byte.
 *   eslam_viewer_begin    clears the keys to all ones;
 *   eslam_viewer_mesh     every fragment does a 64-bit atomicMin into its pixel's key;  (visualizer_util.py:110-115)
 *   eslam_viewer_points   the same for points drawn size x size pixels;                 (visualizer_util.py:57-59, 131-148, 182)
 *   eslam_viewer_resolve  keys -> image [n_views][H][W][3] uint8 and, when depth is not NULL, depth [n_views][H][W]
 *                         float32; untouched pixels get the background colour and depth 0.  (capture_screen_image, :175)
 * Any number of mesh and point calls may fall between begin and resolve, all with the begin's n_views, H, W and workspace.
 * The nearest fragment wins and equal depths go to the smaller colour word, so the image depends neither on the order of
 * the calls nor on the order of execution: bit-identical run to run.
 * Mesh fragments: setup, skipped triangles, pixel box, near-plane rule, edge functions E_k and depth z are those of
 * eslam_raster_depth above (with return of the depth and no culling: the same bits), and so are large_area, the two triangle
 * paths and the queue.  Colour: barycentrics b_k = E_k / ((E_0 + E_1) + E_2) (perspective-correct: E_0 = b_0 det[v0 v1 v2] / z;
 * b = (1, 0, 0) should the sum be 0), per channel c = (b_0 c_0 + b_1 c_1) + b_2 c_2 with c_k the vertex's uint8 as float,
 * clamped to [0, 255], stored as (uint8)floor(c + 0.5); alpha 255.  colors [n_verts][4] uint8 (the PLY's layout, 4-byte
 * aligned, the fourth byte ignored) or NULL = every vertex (200, 200, 200).  cull_backfaces != 0: a triangle with
 * (n . v0) >= 0, n = (v1 - v0) x (v2 - v0) in the camera frame (its normal points away from the camera), emits nothing.
 * Point fragments, float32 operation by operation: c = w2c [p, 1], each row ((m0 x + m1 y) + m2 z) + m3; skipped unless
 * z_near <= c.z <= z_far; u = fx c.x / c.z + cx, v = fy c.y / c.z + cy; x0 = (int)ceil(clamp(u - size / 2, -size, W)),
 * y0 = (int)ceil(clamp(v - size / 2, -size, H)) (fmax first: NaN becomes -size); the point covers the pixels
 * x0 .. x0 + size - 1, y0 .. y0 + size - 1 inside the image, each with the key of c.z and the point's colour, alpha 255.
 * rgba: [n_points][4] uint8 when per_point != 0, else one [4] for the call.  1 <= size <= ESLAM_VIEWER_MAX_POINT_SIZE.
 * workspace: eslam_viewer_workspace_bytes(n_faces, n_views, H, W) bytes for meshes of at most n_faces faces (keys, tile
 * counters, tile queues).  H, W <= 16384.  Zero views, faces or points are valid and launch nothing.  Every call launches on
 * `stream` and never synchronises; bad arguments come back non-zero, with eslam_last_error() set, before any launch.      */
#define ESLAM_VIEWER_MAX_POINT_SIZE 16
int64_t eslam_viewer_workspace_bytes(int64_t n_faces, int n_views, int H, int W);
int eslam_viewer_begin(int n_views, int H, int W, void* workspace, eslam_stream_t stream);
int eslam_viewer_mesh(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const uint8_t* colors,
                      const float* w2c, int n_views, float fx, float fy, float cx, float cy, int H, int W, float z_near,
                      float z_far, int cull_backfaces, int large_area, void* workspace, eslam_stream_t stream);
int eslam_viewer_points(const float* points, int64_t n_points, const uint8_t* rgba, int per_point, int size, const float* w2c,
                        int n_views, float fx, float fy, float cx, float cy, int H, int W, float z_near, float z_far,
                        void* workspace, eslam_stream_t stream);
int eslam_viewer_resolve(int n_views, int H, int W, int bg_r, int bg_g, int bg_b, const void* workspace, uint8_t* image,
                         float* depth, eslam_stream_t stream);

/* Headlight Lambert shading of a mesh's vertex colours for ONE view, applied before rasterisation (the reference's window is
 * unlit; eslam_viewer_mesh and its contract are untouched: hand it `out` as the colours of that view).  verts, normals
 * [n_verts][3] float32 (device; normals need not be unit), colors [n_verts][4] uint8 (4-byte aligned, the fourth byte
 * ignored) or NULL = every vertex (200, 200, 200), cam_center3_host: the camera centre c (host).  Per vertex, float32
 * operation by operation: l = c - v; nn = (nx nx + ny ny) + nz nz and ll likewise; the factor k = 1 when nn == 0 or
 * ll == 0, else k = ambient + (1 - ambient) max(0, ((nx lx + ny ly) + nz lz) / (sqrt(nn) sqrt(ll))); every channel becomes
 * (uint8)floor(min(255, c k) + 0.5) with c the channel's uint8 as float; alpha 255.  out [n_verts][4] uint8, 4-byte aligned.
 * 0 <= ambient <= 1.  Zero vertices are valid and launch nothing; one launch on `stream`, never synchronises; bad arguments
 * come back non-zero, with eslam_last_error() set, before any launch.                                                  */
int eslam_shade_vertices(const float* verts, const float* normals, const uint8_t* colors, int64_t n_verts,
                         const float* cam_center3_host, float ambient, uint8_t* out, eslam_stream_t stream);

/* Render metrics and the frame visualiser's panel (reference src/utils/Frame_Visualizer.py:43-122): three operations on a
 * rendered frame and its ground truth.  depth, gt_depth [H][W]; color, gt_color [H][W][3]; all float32 on the device.
 * Every call launches on `stream` and never synchronises; bad arguments come back non-zero before any launch.
 *
 * eslam_frame_stats: out [4] (device, float64) =
 *   n_valid        the number of pixels with gt_depth > 0
 *   sum_abs_depth  the sum over those pixels of |depth - gt_depth|, the difference taken in float32 and widened to double
 *   sum_sq_color   the sum over all 3 H W colour values of (color - gt_color)^2, unclipped: the difference taken in float32
 *                  and squared in double (Slam.render_quality's mse before the division)
 *   max_gt_depth   the largest gt_depth
 * A two-stage fixed-order tree in float64 (no float atomics): a workgroup per ESLAM_STATS_BLOCK_PIXELS pixels, then one
 * workgroup over the partials; bit-identical run to run.  workspace: eslam_frame_stats_workspace_bytes(H, W) bytes.
 * 1 <= H, W <= 16384.                                                                                              */
#define ESLAM_STATS_BLOCK_PIXELS 4096
int64_t eslam_frame_stats_workspace_bytes(int H, int W);
int eslam_frame_stats(const float* depth, const float* gt_depth, const float* color, const float* gt_color, int H, int W,
                      void* workspace, double* out, eslam_stream_t stream);

/* Mean SSIM (Wang, Bovik, Sheikh, Simoncelli 2004) of two [H][W][C] float32 images a and b, C = 1 or 3.  Inputs are clipped
 * to [0, 1] on load (a NaN reads as 0).  The window is the 11 x 11 Gaussian with sigma = 1.5, w[k] = exp(-(k - 5)^2 / 4.5)
 * normalised to sum 1 in float64 and rounded to float32, applied separably (rows, then columns) over the valid region only,
 * no padding: the map is [H - 10][W - 10][C].  Population moments (no sample-covariance correction), C1 = 1e-4 and
 * C2 = 9e-4 (data range 1).  H < 11 or W < 11 (or > 16384), or another C, is an argument error.
 * One output tile of ESLAM_SSIM_TILE_H x ESLAM_SSIM_TILE_W pixels of one channel per workgroup: the tile and its 10-pixel
 * halo of both images staged in LDS, the horizontal pass of the five moment images into LDS, the vertical pass and the
 * formula in registers.  float32 variances are differences of nearly equal numbers, so the moments are taken of values
 * shifted by a per-tile constant (variances and covariances do not depend on it).  Operation order, float32 and unfused,
 * every window sum running k = 0 .. 10 as acc = w[0] v[0], then acc = acc + w[k] v[k]:
 *   kx, ky = clip(a), clip(b) at the tile's first pixel (its top-left output position, same channel)
 *   x = clip(a) - kx,  y = clip(b) - ky
 *   h_x, h_y, h_xx, h_yy, h_xy = sum_k w[k] {x, y, x x, y y, x y}[r][j + k]
 *   m_x, m_y, m_xx, m_yy, m_xy = sum_k w[k] h_*[i + k][j]
 *   vx = m_xx - m_x m_x,  vy = m_yy - m_y m_y,  vxy = m_xy - m_x m_y,  ux = kx + m_x,  uy = ky + m_y
 *   ssim = ((2 (ux uy) + C1) (2 vxy + C2)) / ((ux ux + uy uy + C1) (vx + vy + C2)), a true division
 * map [H - 10][W - 10][C] float32 may be NULL.  mean [1] (device, float64) = the sum of the float32 map values by a
 * fixed-order float64 tree (per tile, then over the tiles), divided by their number: bit-identical run to run.
 * workspace: eslam_ssim_workspace_bytes(H, W, C) bytes (-1 for a shape eslam_ssim refuses).                          */
#define ESLAM_SSIM_TILE_H 16
#define ESLAM_SSIM_TILE_W 32
int64_t eslam_ssim_workspace_bytes(int H, int W, int C);
int eslam_ssim(const float* a, const float* b, int H, int W, int C, void* workspace, float* map, double* mean,
               eslam_stream_t stream);

/* out [2 H][3 W][3] uint8: the visualiser's 2 x 3 panel at the frame's own resolution.
 * Row 0: gt_depth, depth, and |gt_depth - depth| forced to 0 where gt_depth == 0, each through the colour map:
 *   vmax = float(stats[3]) read on the device (eslam_frame_stats' out), 1 when it is 0;  t = v / vmax, a true float32
 *   division;  LUT index 0 for t <= 0 or NaN, otherwise min(255, int(t 256));  lut [256][3] uint8 on the device (plasma).
 * Row 1: gt_color, color, and |gt_color - color| forced to 0 where gt_depth == 0, each clipped to [0, 1] (a NaN reads as
 *   0), then uint8(c 255 + 0.5f): a float32 multiplication, then a float32 addition, truncated.                     */
int eslam_vis_panel(const float* depth, const float* gt_depth, const float* color, const float* gt_color, int H, int W,
                    const double* stats, const uint8_t* lut, uint8_t* out, eslam_stream_t stream);

/* check_proj (src/tools/eval_recon.py:59-85) for a chunk of n_views candidate views: seen[k] (uint8, ORed into: set
 * to 1, never cleared) when any point of points [n_points,3] projects into view k.  w2c [n_views][12]: the 3x4 rows
 * (float32) of the float64 inverse, taken on the host, of c2w[k] with its columns 1 and 2 negated (eval_recon.py:64-68).
 * For point p and view k, in float32:
 *   c = w2c[k] [p, 1];  c.x *= -1;  a = fx c.x + cx c.z;  b = fy c.y + cy c.z;  z = c.z + 1e-5;  u = a / z;  v = b / z;
 *   p is in view when 0 <= -z, 0 < u < W and 0 < v < H                                         (edge = 0).          */
int eslam_views_see_points(const float* points, int64_t n_points, const float* w2c, int n_views, float fx, float fy,
                           float cx, float cy, int H, int W, uint8_t* seen, eslam_stream_t stream);

/* Backward of eslam_decode_fwd: g_raw [N,4] upstream, raw [N,4] the forward output.  Same gradient outputs as
 * eslam_render_bwd, with g_pts [N,3] (may be NULL) instead of ray gradients.  Planes that carry data_f16: the mixed-precision
 * path, as in eslam_render_bwd - feat is what eslam_decode_fwd saved on the same planes ([N,128] bf16), g_pts is taken on the
 * half copies, plane gradients accumulate in float32 into `grad`.                                          */
int eslam_decode_bwd(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                     const float* pts, int64_t N, const float* raw, const float* feat, const float* g_raw,
                     float* g_dec, float* g_pts, void* workspace, eslam_stream_t stream);

/* Caller-side loss of one optimisation iteration, value and upstream gradients in two small launches and
 * without the boolean-mask host syncs of the PyTorch formulation.  Replaces src/Mapper.py:110-144 (sdf_losses)
 * + :337-346, and src/Tracker.py:114-148 + :197-204 when ray_mask is given.
 *   ray_mask == NULL: every ray belongs to the batch.
 *   ray_mask != NULL: uint8 [R], the rays that belong to the batch - the 10x-median outlier mask of
 *                     Tracker.py:193-195, and/or the AABB pre-filter of Mapper.py:322-332 / Tracker.py:175-187 kept
 *                     as a mask instead of a compaction (no host sync, static shapes for hipGraph capture).
 *   Colour term: mean over the batch's rays; SDF and depth terms: mean over the batch's rays with gt_depth > 0
 *   (in tracking the pre-filter already requires depth, so all three run over the same rays, as the reference's do).
 * weights5_host = {w_sdf_fs, w_sdf_center, w_sdf_tail, w_depth, w_color}  (configs/ESLAM.yaml:29-33,53-57).
 * Outputs: loss [1]; g_depth [R], g_rgb [R,3], g_sdf [R,S] = d loss / d (depth, rgb, sdf) (overwritten).
 * Means over empty sets give NaN exactly as torch.mean does.  scratch: 64 bytes, any contents.            */
int eslam_mapping_loss(const float* depth, const float* rgb, const float* sdf, const float* z_vals,
                       const float* gt_depth, const float* gt_color, int R, int S, double truncation,
                       const float* weights5_host, const uint8_t* ray_mask, float* loss,
                       float* g_depth, float* g_rgb, float* g_sdf, void* scratch, eslam_stream_t stream);

/* The two phases of eslam_mapping_loss separately, for ray-sharded data parallelism: every rank runs
 * eslam_loss_reduce on its shard, the ESLAM_LOSS_ACC floats of `acc` (set sizes and squared-error sums) are
 * summed over ranks with one tiny all-reduce, then eslam_loss_grad produces upstream gradients scaled by the GLOBAL
 * set sizes, so the summed gradients equal those of the unsharded batch.  acc must be zeroed by the caller
 * before eslam_loss_reduce (it accumulates).  eslam_loss_grad: loss, g_* may be NULL when not wanted; `upstream`
 * (device scalar, optional) multiplies the gradients - the grad_output autograd hands to the loss's backward.    */
#define ESLAM_LOSS_ACC 16
int eslam_loss_reduce(const float* depth, const float* rgb, const float* sdf, const float* z_vals,
                      const float* gt_depth, const float* gt_color, int R, int S, double truncation,
                      const uint8_t* ray_mask, float* acc, eslam_stream_t stream);
int eslam_loss_grad(const float* depth, const float* rgb, const float* sdf, const float* z_vals,
                    const float* gt_depth, const float* gt_color, int R, int S, double truncation,
                    const float* weights5_host, const uint8_t* ray_mask, const float* acc, float* loss,
                    float* g_depth, float* g_rgb, float* g_sdf, const float* upstream, eslam_stream_t stream);

/* Optimiser step of the callers' loops: torch.optim.Adam exactly as the reference
 * builds it - default betas (0.9, 0.999) and eps 1e-8 unless given, no weight decay, no amsgrad - over all
 * parameter tensors of one step in ONE launch.  Replaces `optimizer.step()` (+ optionally `optimizer.zero_grad()`)
 * of src/Mapper.py:291-303,348-350 (decoders / planes / c_planes / camera-pose groups, one lr each) and of
 * src/Tracker.py:262-266,206-208 (cam_pose translation / rotation groups).
 *   tensors_host: HOST array of n_tensors descriptors; each names four dense device arrays of n float32 in the
 *                 same element order (param, grad, exp_avg, exp_avg_sq) and the lr of the tensor's param group;
 *   step:         1-based step count t of the bias corrections (state['step'] after the increment), used when
 *                 step_dev is NULL;
 *   step_dev:     optional device int32 counter: incremented by one on the stream and then used as t, so that a
 *                 captured hipGraph can be replayed without re-recording (t never appears in the kernel arguments);
 *   zero_grad:    non-zero = clear every consumed gradient in the same pass.
 * Elements whose grad, exp_avg and exp_avg_sq are all zero are skipped - the dense update leaves them unchanged
 * bit for bit.  Tensors whose four pointers are 16-byte aligned take the float4 path.                          */
#define ESLAM_ADAM_MAX_TENSORS 32   /* descriptors per launch; longer tables are split into several launches */
typedef struct {
    float* param;
    float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;
    double lr;
} eslam_adam_tensor_t;
int eslam_adam_step(const eslam_adam_tensor_t* tensors_host, int n_tensors, int step, int32_t* step_dev,
                    double beta1, double beta2, double eps, int zero_grad, eslam_stream_t stream);

/* Keyframe selection by view overlap, the projection test of src/Mapper.py:170-201 for all keyframes in one launch:
 * the current frame's rays (get_samples, Mapper.py:166-168) with depth > 0 are sampled at num_samples depths between
 * 0.8 d and d + 0.5, projected into each keyframe (w2c = inverse(c2ws[k]), x flipped, pinhole K) and counted when they
 * fall inside the image less `edge` pixels with negative camera z.
 *   c2ws [n_keyframes,4,4] row-major camera-to-world (the caller drops the last two keyframes, Mapper.py:183);
 *   counts int32 [n_keyframes + 1]: counts[k] = points inside keyframe k; counts[n_keyframes] = rays with depth > 0,
 *   so percent_inside[k] = counts[k] / (counts[n_keyframes] * num_samples)  (Mapper.py:201).                     */
int eslam_keyframe_overlap(const float* rays_o, const float* rays_d, const float* gt_depth, int n_rays,
                           int num_samples, const float* c2ws, int n_keyframes, int H, int W, float fx, float fy,
                           float cx, float cy, int edge, int32_t* counts, eslam_stream_t stream);

/* Caller-side glue of the optimisation loops, one launch each instead of a chain of small tensor ops.
 *
 * eslam_prefilter: keep[i] = (AABB exit distance of ray i >= gt_depth[i]) [&& gt_depth[i] > 0 when need_depth]
 *   - the pre-filter of src/Mapper.py:322-328 (need_depth = 0) and src/Tracker.py:175-182 (need_depth = 1) as a uint8
 *   mask for the `ray_mask` of the loss entry points, instead of a boolean-index compaction.
 * eslam_pose_to_c2w(_bwd): src/common.py:169-181 cam_pose_to_matrix - poses [b,7] = (quaternion real-first, translation)
 *   -> c2ws [b,4,4] with R = quaternion_to_matrix(q) (q need not be normalised: two_s = 2 / |q|^2) - and its
 *   backward g_c2ws [b,4,4] -> g_poses [b,7].
 * eslam_tracking_mask: src/Tracker.py:192-195.  mask[i] = keep[i] && |gt_depth[i] - depth[i]| < factor * median, the
 *   (lower, as torch.median) median taken over the rays with keep[i] != 0 (all rays when keep is NULL); R <=
 *   ESLAM_TRACKING_MASK_MAX.  A NaN error makes the median NaN and the mask empty, as in the reference.
 * eslam_keep_best: src/Tracker.py:304-307.  if (loss[0] < best[0]) { best[0] = loss[0]; best_pose[0..n) = pose[0..n); } */
#define ESLAM_TRACKING_MASK_MAX 8192
int eslam_prefilter(const float* rays_o, const float* rays_d, const float* gt_depth, int R, const float* bound6_host,
                    int need_depth, uint8_t* keep, eslam_stream_t stream);
int eslam_pose_to_c2w(const float* poses, int b, float* c2ws, eslam_stream_t stream);
int eslam_pose_to_c2w_bwd(const float* poses, const float* g_c2ws, int b, float* g_poses, eslam_stream_t stream);
int eslam_tracking_mask(const float* depth, const float* gt_depth, const uint8_t* keep, int R, float factor,
                        uint8_t* mask, eslam_stream_t stream);
int eslam_keep_best(const float* loss, const float* pose, int n, float* best, float* best_pose,
                    eslam_stream_t stream);

/* Single-GPU forward of the fused loss in ONE launch: the sums of eslam_loss_reduce, acc [ESLAM_LOSS_ACC] (overwritten -
 * no pre-zeroing) and the loss value [1] (may be NULL).  scratch: ESLAM_LOSS_SCRATCH floats that the caller zeroes ONCE
 * when allocating them and then only hands to this function (it holds a self-resetting ticket counter and the
 * running sums, one cache line each; one scratch per concurrently running stream).  eslam_loss_grad(acc) gives the gradients. */
#define ESLAM_LOSS_SCRATCH (32 * 17)
/* Size (floats) of the scratch for a batch of n_rays: ESLAM_LOSS_SCRATCH, or more in deterministic mode.
 * eslam_deterministic(): 1 when the process runs with ESLAM_DETERMINISTIC=1 - the loss's sums are then reduced in a fixed
 * order (per-workgroup slots instead of float atomics) and the plane-gradient scatter accumulates in 64-bit fixed point
 * (integer adds commute), so every output of the path is bitwise reproducible from run to run, at a lower speed.
 * Range of the fixed-point sums: units of 2^-44, so one contribution must stay below 2^18 = 2.6e5 in magnitude and a texel's
 * sum below 5.2e5; a contribution beyond the limit, or a NaN / Inf one, poisons the float gradient of the texels it goes to
 * (and of no other texel) with NaN instead of being saturated silently.  A sum that leaves the range while every contribution
 * is inside it wraps undetected.  One int64 shadow of the planes per device, allocated at the first (eager) use.
 * eslam_loss_scratch_reset: back to the freshly-zeroed state, e.g. after a graph was aborted mid-flight.             */
int eslam_deterministic(void);
/* Samples per workgroup (1024 or 2048) the plane-gradient scatter uses for a batch of n rays with S samples each (render != 0)
 * or of n free points (render == 0, S ignored): 2048, except in the default mode for batches that would make fewer than 192
 * workgroups of 2048 samples.  Host arithmetic only, no launch; 0 for an empty or invalid batch. */
int eslam_scatter_bundle_samples(int64_t n, int S, int render);
/* Which pair of kernels the last eslam_render_bwd / eslam_render_bwd_loss / eslam_decode_bwd of this process dispatched:
 * 1 = the rank-16 pair (float32 planes with gradients, rays without position gradients, not deterministic mode: the decoder
 * backward stores the 16-wide hidden gradient, the scatter expands it per cell), 0 = full-width feature-gradient rows.
 * Host bookkeeping, no launch.  FOR TESTS ONLY: one unsynchronised process-wide value written at dispatch - with concurrent
 * callers it is racy and names only the last dispatch; no caller may branch on it. */
int eslam_last_backward_rank16(void);
/* The rank-16 scatter's paired grid: where the SDF decoder's plane and the colour decoder's of one (orientation, level) -
 * planes p and p + 6 - agree in width, height and strides and both receive gradients, one workgroup per bundle sorts the
 * bundle's cells once and walks them twice; the other planes keep a workgroup each (the reference's default shapes agree at the
 * coarse level only: three pairs, six single planes).  With no agreeing pair the 12-plane grid is used.
 * eslam_scatter_pairing(mode): 0 = never, 1 = auto (the default: pair when bundles x (12 - pairs) >= 3 x the device's compute
 * units - smaller batches want more workgroups, not fewer), 2 = whenever a pair agrees; returns the previous mode, an invalid
 * mode changes nothing.  A process-wide host-side value read at launch - FOR TESTS AND MEASUREMENTS, set it while no other
 * thread launches.
 * eslam_last_scatter_paired(): 1 if the last scatter launch of this process used the paired grid.  Host bookkeeping, FOR TESTS
 * ONLY, racy with concurrent callers like eslam_last_backward_rank16.
 * eslam_scatter_pairs_auto(n, S, cus, npairs): what the auto rule decides for n rays of S samples, npairs (1..6) of whose plane
 * pairs agree, on a device of `cus` compute units.  Host arithmetic only, no launch. */
int eslam_scatter_pairing(int mode);
int eslam_last_scatter_paired(void);
int eslam_scatter_pairs_auto(int64_t n, int S, int cus, int npairs);
/* The same kind of bookkeeping, FOR TESTS ONLY: 1 = that backward read the forward pass's saved first hidden layer
 * (eslam_render_bwd_h / _bwd_loss_h with a buffer, float32 planes), 0 = it recomputed the layer from the features. */
int eslam_last_backward_saved_hidden(void);

/* Host-side helper of the Python layer (no reference counterpart): `waiter` waits for the work enqueued on `signaler` so
 * far - the fork / join of the side stream the ray ordering (eslam_ray_order, what the backward's scatter bundles by) runs
 * on beside the samplers and the forward kernel.  One hipEventRecord + hipStreamWaitEvent; valid inside a stream capture. */
int eslam_stream_wait(eslam_stream_t waiter, eslam_stream_t signaler);

/* Host-side helper: zero `bytes` bytes at `ptr` on `stream`.  The gradient buffer autograd hands to the optimiser has to be
 * zero before the scatter adds into it (the reference's `fill_` of the plane gradients is 15.9 % of its CPU step, SURVEY.md
 * section 8a6); cleared at the head of the side stream it runs beside the samplers. */
int eslam_zero_async(void* ptr, int64_t bytes, eslam_stream_t stream);
int64_t eslam_loss_scratch_floats(int64_t n_rays);
int eslam_loss_scratch_reset(float* scratch, int64_t floats, eslam_stream_t stream);
int eslam_loss_value(const float* depth, const float* rgb, const float* sdf, const float* z_vals,
                     const float* gt_depth, const float* gt_color, int R, int S, double truncation,
                     const float* weights5_host, const uint8_t* ray_mask, float* scratch, float* acc, float* loss,
                     eslam_stream_t stream);

/* Per-kernel device timing for bench.py's roofline line (HIP events recorded on the launch stream around each
 * kernel while enabled; adds nothing to the launch path when disabled).  Usage: enable(1); run one iteration;
 * synchronise the stream; read(ms) -> elapsed milliseconds of the LAST launch of each kernel, -1 if it did not run. */
#define ESLAM_PROF_KERNELS 13
int eslam_profile_enable(int on);
int eslam_profile_read(float* ms_out);
const char* eslam_profile_name(int kernel_id);

/* Ray-sharded mapping iteration WITHOUT a collective between forward and backward (round 3; SURVEY.md section 8(e):
 * "compute them redundantly on every rank").  Every rank holds the iteration's whole batch of rays (same get_samples draw,
 * src/Mapper.py:318-319) and renders its slice; what the backward needs from the other ranks' rays it computes itself:
 *
 * eslam_loss_set_sizes: the five set sizes the mapping loss takes its means over (src/Mapper.py:136-140,343,346) for all R
 *   rays of the batch, without rendering them - they depend on gt_depth, ray_mask and the depth-guided z_vals of the rays
 *   with depth only (src/utils/Renderer.py:85-105), which the kernel replays in LDS with the sampler's own arithmetic and
 *   random numbers (t_rand [R,S] injected, or NULL = the in-kernel numbers of eslam_sample_z_all_rng for seed / rng_state /
 *   global ray index).  acc_out [ESLAM_LOSS_ACC]: the count slots as floats, other slots 0 - hand it to
 *   eslam_render_bwd_loss as `acc`.  scratch: 7 x 32 uint32, zeroed once by the caller, left zeroed.
 * eslam_mark_rays: touched [n_blocks] (cleared here) <- 1 for every texel that CAN receive gradient from the batch's rays,
 *   from ray geometry alone: the samples of a ray with depth d lie in [min(0, d - 1.5 tau), max(1.2 d, d + 1.5 tau)], those of
 *   a depth-less ray between 0 and far = AABB exit + 0.01 (Renderer.py:96-100,114-134), that is in the ORDERED interval
 *   [min(0, far), max(0, far)]: far is negative for a ray that starts outside the bound and points away from it.  The
 *   interval is ordered first and padded (by 1e-5 of its ends + 1e-6) second, its length enters as |hi - lo|, and at least
 *   one step is taken; the segment is rasterised conservatively into each plane.  A ray whose far is not finite is marked by
 *   its clamped box in one step.  A superset of the texels the ranks' backward passes add to, identical on every rank,
 *   known before anything is sampled.  channels_last planes only (one block = one texel's 32 channels = 128 bytes of the flat gradient buffer);
 *   block_base_host[12] = index of each plane's first block in that buffer.
 * eslam_blocks_compact: idx [n_blocks capacity] <- ascending indices of the non-zero bytes of touched; meta[0] <- their
 *   number, meta[1] += 1 (a stamp: the host compares it with its own count of launches before it sizes the all-reduce).
 *   host_meta_dev (optional): the device address of two int32 of pinned host memory (eslam_host_meta_alloc) that receive
 *   the same two words straight from the kernel - no copy node.  clear_touched: zero the bytes behind the read, so that the
 *   next iteration's marking needs no memset.  scratch: eslam_blocks_compact_scratch_words(n_blocks) uint32, zeroed once.
 * eslam_shard_prologue: the clear of the previous iteration's gradients (eslam_blocks_zero_dev; clear_flat NULL = none), the
 *   set sizes (eslam_loss_set_sizes, in-kernel random numbers) and the marking (eslam_mark_rays WITHOUT its memset: touched
 *   must be clean - eslam_blocks_compact(clear_touched = 1) leaves it so; mark_planes NULL = none) as ONE launch: a replayed
 *   hipGraph pays ~3 us per node, and this work sits beside the sampler and the forward kernel.
 * eslam_blocks_pack_dev / _unpack_dev / _zero_dev: gather the listed blocks of `flat` and the dense `tail` (decoder / beta /
 *   pose gradients, loss sums) into buf / write the all-reduced buf back / zero them, with the list's length read on the
 *   device (meta[0]) and the dense tail FIRST: buf = [tail_pad floats (n_tail used, rest 0; tail_pad % 4 == 0) | 32 floats per
 *   listed block], so that the all-reduce covers buf[0 : tail_pad + 32 meta[0]] of a fixed-capacity buffer.  step_bump
 *   (pack, optional): a device counter the launch increments - a ray-sharded iteration keeps its random-number step there
 *   (rng_state of eslam_sample_z_all_rng and eslam_shard_prologue, which read it on two streams) and advances it with its
 *   last launch instead of through eslam_render_fwd*'s rng_bump.                                                       */
int eslam_loss_set_sizes(const float* gt_depth, const uint8_t* ray_mask, int R, int n_strat, int n_imp, double truncation,
                         const float* t_free, const float* t_surf, const float* t_rand, int perturb, uint64_t seed,
                         const uint32_t* rng_state, uint32_t* scratch, float* acc_out, eslam_stream_t stream);
int eslam_mark_rays(const eslam_plane_t* planes, const float* bound6_host, const float* rays_o, const float* rays_d,
                    const float* gt_depth, int R, double truncation, const int64_t* block_base_host, int64_t n_blocks,
                    uint8_t* touched, eslam_stream_t stream);
int64_t eslam_blocks_compact_scratch_words(int64_t n_blocks);
int eslam_blocks_compact(uint8_t* touched, int64_t n_blocks, uint32_t* scratch, int32_t* idx, int32_t* meta,
                         int32_t* host_meta_dev, int clear_touched, eslam_stream_t stream);
int eslam_host_meta_alloc(void** host_ptr, void** dev_ptr);
int eslam_host_meta_free(void* host_ptr);
int eslam_shard_prologue(float* clear_flat, const int32_t* clear_idx, const int32_t* clear_meta, int64_t clear_capacity,
                         float* clear_tail, int64_t clear_n_tail, const float* rays_o, const float* rays_d,
                         const float* gt_depth, const uint8_t* ray_mask, int R, int n_strat, int n_imp, double truncation,
                         const float* t_free, const float* t_surf, int perturb, uint64_t seed, const uint32_t* rng_state,
                         uint32_t* sizes_scratch, float* acc_out, const eslam_plane_t* mark_planes, const float* bound6_host,
                         const int64_t* block_base_host, int64_t n_blocks, uint8_t* touched, eslam_stream_t stream);
int eslam_blocks_pack_dev(const float* flat, const int32_t* idx, const int32_t* meta, int64_t capacity, const float* tail,
                          int64_t n_tail, int64_t tail_pad, float* buf, uint32_t* step_bump, eslam_stream_t stream);
int eslam_blocks_unpack_dev(float* flat, const int32_t* idx, const int32_t* meta, int64_t capacity, float* tail,
                            int64_t n_tail, int64_t tail_pad, const float* buf, eslam_stream_t stream);
int eslam_blocks_zero_dev(float* flat, const int32_t* idx, const int32_t* meta, int64_t capacity, float* tail, int64_t n_tail,
                          eslam_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ESLAM_HIP_H */
