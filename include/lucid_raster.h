/*
 * lucid_raster.h -- C-ABI of the MI355X-native differentiable Gaussian-splat rasterizer.
 *
 * This is the drop-in boundary under LucidDreamer's `depth_diff_gaussian_rasterization_min`
 * extension.  Each entry point replaces one static method of the reference's
 * CudaRasterizer::Rasterizer (RAST/ = /root/reference/submodules/depth-diff-gaussian-rasterization-min/):
 *
 *   lr_forward       <->  Rasterizer::forward      RAST/cuda_rasterizer/rasterizer.h:31-55,
 *                                                  RAST/cuda_rasterizer/rasterizer_impl.cu:198-339
 *   lr_backward      <->  Rasterizer::backward     RAST/cuda_rasterizer/rasterizer.h:57-86,
 *                                                  RAST/cuda_rasterizer/rasterizer_impl.cu:343-444
 *   lr_mark_visible  <->  Rasterizer::markVisible  RAST/cuda_rasterizer/rasterizer.h:24-29,
 *                                                  RAST/cuda_rasterizer/rasterizer_impl.cu:141-153
 *   lr_dist2         <->  SimpleKNN::knn           /root/reference/submodules/simple-knn/simple_knn.h,
 *                                                  simple_knn.cu:186-221 (distCUDA2, spatial.cu:15-26)
 *
 * Plain pointers and sizes only (no torch types).  All pointers are DEVICE pointers (HBM) unless
 * stated otherwise; all arrays are dense row-major float32/int32 exactly as the reference lays
 * them out.  Differences from the reference signature, all additive:
 *   - the three std::function<char*(size_t)> allocators become C callbacks + a user cookie;
 *   - every call takes the HIP stream to enqueue on (the reference uses the legacy default stream);
 *   - lr_forward takes `binning_capacity` (see below) to run WITHOUT the per-view host sync;
 *   - errors are returned as negative codes (lr_last_error() gives the text) instead of C++
 *     exceptions / device traps;
 *   - gradient outputs of lr_backward need NOT be zero-filled by the caller.
 *
 * Optional inputs (shs / colors_precomp, scales+rotations / cov3D_precomp) are NULL when absent
 * (the reference tests the pointer for nullptr: forward.cu:205,241; backward.cu:390,394).
 */
#ifndef LUCID_RASTER_H_INCLUDED
#define LUCID_RASTER_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Allocator callback: must return a device pointer to at least `bytes` bytes, 256-byte aligned,
 * that stays valid until the matching lr_backward has completed
 * (replaces std::function<char*(size_t)>, RAST/rasterize_points.cu:27-33). */
typedef char* (*lr_alloc_fn)(size_t bytes, void* user);

/* Error codes (negative return values). */
#define LR_ERR_INVALID_ARG   (-10)  /* bad shapes / NULL required pointer / non-RGB (rasterizer_impl.cu:243-246) */
#define LR_ERR_HIP           (-11)  /* a HIP runtime call failed (debug => after a stream sync, auxiliary.h:166-173) */
#define LR_ERR_PREFILTERED   (-12)  /* "Point is filtered although prefiltered is set" (auxiliary.h:156-160) */
#define LR_ERR_OVERFLOW      (-13)  /* async mode: num_rendered exceeded binning_capacity */
#define LR_ERR_ALLOC         (-14)  /* allocator callback returned NULL */
#define LR_NUM_RENDERED_ON_DEVICE (-1) /* lr_forward return value in async mode */

/* lr_backward accumulate_mask bits (one per gradient output, in argument order) */
#define LR_ACC_MEAN2D  (1u << 0)
#define LR_ACC_CONIC   (1u << 1)
#define LR_ACC_OPACITY (1u << 2)
#define LR_ACC_COLOR   (1u << 3)
#define LR_ACC_MEAN3D  (1u << 4)
#define LR_ACC_COV3D   (1u << 5)
#define LR_ACC_SH      (1u << 6)
#define LR_ACC_SCALE   (1u << 7)
#define LR_ACC_ROT     (1u << 8)
/* write-mode outputs: rows of Gaussians without a tile instance stay UNWRITTEN instead of zero-filled (see lr_adam_step_masked) */
#define LR_ACC_NO_ZERO_FILL (1u << 31)

const char* lr_last_error(void);
const char* lr_version(void);

/* Scratch sizes (bytes).  geom depends on P only, img on W,H only, binning on the number of
 * tile instances R (num_rendered) -- cf. required<GeometryState/ImageState/BinningState>,
 * RAST/cuda_rasterizer/rasterizer_impl.cu:226, 239, 284. */
size_t lr_geom_bytes(int P);
size_t lr_img_bytes(int width, int height);
size_t lr_binning_bytes(long long R);

/*
 * Forward.  Returns num_rendered (>= 0) in exact mode, LR_NUM_RENDERED_ON_DEVICE in async mode,
 * or a negative LR_ERR_*.
 *
 * binning_capacity == 0  (exact mode, reference behaviour): after the tile-count scan the host
 *     reads num_rendered back (one 4-byte D2H + stream sync, as rasterizer_impl.cu:281-282) and
 *     sizes the binning buffer exactly.
 * binning_capacity  > 0  (async mode): no host synchronisation at all.  The binning buffer is
 *     sized for `binning_capacity` tile instances; num_rendered stays in the geom buffer header.
 *     If the view needs more, nothing is written out of bounds, the overflow flag in the header
 *     is set and lr_check (or lr_views_check for the multi-view entry points) returns LR_ERR_OVERFLOW.  The HOST side
 *     of lr_backward does not look at the flag (it would cost a synchronisation), its KERNELS do: the backward of an
 *     overflowed view writes nothing -- its gradients are zero (write mode) or it adds nothing (accumulate mode); a
 *     truncated instance list is never differentiated.  Callers that need that view's gradients call lr_check after
 *     the step and run the view again with binning_capacity = 0 (the Python operator does this by itself).
 *
 * out_color [3,H,W], out_depth [1,H,W], radii [P] are fully written (no pre-fill needed).
 */
int lr_forward(lr_alloc_fn geom_alloc, void* geom_user,
               lr_alloc_fn binning_alloc, void* binning_user,
               lr_alloc_fn img_alloc, void* img_user,
               int P, int D, int M,
               const float* background,
               int width, int height,
               const float* means3D,
               const float* shs,
               const float* colors_precomp,
               const float* opacities,
               const float* scales,
               float scale_modifier,
               const float* rotations,
               const float* cov3D_precomp,
               const float* viewmatrix,
               const float* projmatrix,
               const float* cam_pos,
               float tan_fovx, float tan_fovy,
               int prefiltered,
               float* out_color,
               float* out_depth,
               int* radii,
               int debug,
               long long binning_capacity,
               void* stream);

/*
 * Backward.  R is the value lr_forward returned and binning_capacity the value it was given
 * (exact mode: R >= 0, capacity 0; async mode: R = LR_NUM_RENDERED_ON_DEVICE, capacity > 0; no host
 * synchronisation happens in either mode -- use lr_check to learn about an overflow).  As in the reference, whose backward lays the
 * binning state out from R (rasterizer_impl.cu:364-366), these two values ARE used: they bound the number of list segments the
 * blend backward launches workgroups for (one per 256 instances of a tile's list beyond its first 256).  (Library versions up
 * to 0.3 accepted and ignored them.)  A call whose values are SMALLER than its forward's may leave listed segments without a
 * workgroup: the kernel notices, the view's gradients are incomplete, and the condition is reported as LR_ERR_INVALID_ARG by
 * lr_check on the view's geom buffer and, with debug != 0, by lr_backward itself.  Larger values only cost idle workgroups;
 * R = LR_NUM_RENDERED_ON_DEVICE with capacity 0 ("unknown") selects kernels that are correct for any launch size.
 * dL_depths is accepted and ignored, exactly as the reference does
 * (RAST/cuda_rasterizer/backward.cu:457-464, 539-554 are commented out); lr_view_backward below honours it.
 * accumulate_mask: bit k set (LR_ACC_*) => that output is ACCUMULATED into (rows of visible Gaussians are
 * added to the existing contents, rows of culled Gaussians are not touched); bit clear => the output is
 * fully written (zero rows for culled Gaussians), no pre-fill needed.  0 reproduces the reference contract.
 * Every gradient output pointer (in either mode) must be 16-byte aligned: the kernels use 16-byte vector
 * accesses on them; a misaligned pointer is rejected with LR_ERR_INVALID_ARG.
 * Outputs:
 *   dL_dmean2D [P,3] (z = 0), dL_dconic [P,4] (slots x,y,w; may be NULL), dL_dopacity [P],
 *   dL_dcolor [P,3], dL_dmean3D [P,3], dL_dcov3D [P,6], dL_dsh [P,M,3] (NULL iff shs NULL),
 *   dL_dscale [P,3], dL_drot [P,4] (written as zeros when cov3D_precomp is used).
 * Intermediate outputs the caller does not need may be NULL: dL_dconic always; dL_dcolor unless
 * colors_precomp is given; dL_dcov3D unless cov3D_precomp is given; dL_dscale/dL_drot unless scales is given.
 * Returns 0 or a negative LR_ERR_*.
 */
int lr_backward(int P, int D, int M, int R,
                const float* background,
                int width, int height,
                const float* means3D,
                const float* shs,
                const float* colors_precomp,
                const float* scales,
                float scale_modifier,
                const float* rotations,
                const float* cov3D_precomp,
                const float* viewmatrix,
                const float* projmatrix,
                const float* campos,
                float tan_fovx, float tan_fovy,
                const int* radii,
                char* geom_buffer,
                char* binning_buffer,
                char* image_buffer,
                const float* dL_dpix,
                const float* dL_depths,
                float* dL_dmean2D,
                float* dL_dconic,
                float* dL_dopacity,
                float* dL_dcolor,
                float* dL_dmean3D,
                float* dL_dcov3D,
                float* dL_dsh,
                float* dL_dscale,
                float* dL_drot,
                int debug,
                long long binning_capacity,
                unsigned int accumulate_mask,
                void* stream);

/*
 * The per-view entries proper: lr_view_forward / lr_view_backward take one argument struct each.  lr_forward / lr_backward above
 * are thin wrappers that fill these structs (activated parameters, no depth / alpha / absgrad mode); everything they document --
 * exact and async mode, R / binning_capacity, accumulate_mask, the 16-byte alignment of the gradient outputs, which outputs may be
 * NULL -- holds here.  No switch selects a mode: which pointers are non-NULL does.  (The positional lr_forward_raw and
 * lr_backward_{raw,depth,alpha,absgrad}* entry points of library versions up to 0.6.1, two per mode, are gone.)
 *
 * lr_view: the scene and camera of one view, shared by its forward and its backward.
 *   raw == 0: the ACTIVATED parameters, field for field the arguments of lr_forward; sh_rest must be NULL; `opacities` is read by
 *     the forward only.
 *   raw != 0: the raw-parameter fast path (no counterpart in the reference's native code).  The reference's
 *     Python caller materialises the activated parameters for every view before calling the rasterizer -- exp(scaling),
 *     normalize(rotation), sigmoid(opacity) and torch.cat(features_dc, features_rest) (R/scene/gaussian_model.py:97-117,
 *     R/gaussian_renderer/__init__.py:53-80): a 192 B/Gaussian copy plus four elementwise kernels forward, and their autograd
 *     counterparts backward.  In this mode the fields hold the STORED GaussianModel tensors and the per-Gaussian kernels apply the
 *     activations (forward) and their derivatives (backward):
 *       means3D = xyz [P,3]; shs = features_dc [P,1,3]; sh_rest = features_rest [P,M-1,3] (NULL iff M == 1);
 *       opacities = opacity_raw [P,1] (pre-sigmoid; also read by the backward); scales = scaling_raw [P,3] (pre-exp);
 *       rotations = rotation_raw [P,4] (pre-normalisation, torch.nn.functional.normalize eps 1e-12).
 *     M = 1 + number of rest coefficients (>= 1); D as in lr_forward.  colors_precomp, cov3D_precomp and prefiltered do not exist
 *     in this mode (LR_ERR_INVALID_ARG when given).  The scratch buffers of a raw forward must be used with a raw backward.
 */
typedef struct lr_view {
    /* sizes and the parameter representation (see above) */
    int P, D, M;
    int raw;
    /* the image */
    const float* background;
    int width, height;
    /* the scene: shs or colors_precomp; scales + rotations or cov3D_precomp */
    const float* means3D;
    const float* shs;
    const float* sh_rest;
    const float* colors_precomp;
    const float* opacities;
    const float* scales;
    float scale_modifier;
    const float* rotations;
    const float* cov3D_precomp;
    /* the camera */
    const float* viewmatrix;
    const float* projmatrix;
    const float* campos;
    float tan_fovx, tan_fovy;
} lr_view;

typedef struct lr_forward_args {
    size_t struct_bytes;                     /* = sizeof(lr_forward_args); anything else is LR_ERR_INVALID_ARG */
    lr_view view;
    /* scratch allocators, as in lr_forward */
    lr_alloc_fn geom_alloc;    void* geom_user;
    lr_alloc_fn binning_alloc; void* binning_user;
    lr_alloc_fn img_alloc;     void* img_user;
    int prefiltered;                         /* must be 0 in raw mode */
    /* outputs, fully written: colour [3,H,W], depth [1,H,W], radii [P] */
    float* out_color;
    float* out_depth;
    int* radii;
    int debug;
    long long binning_capacity;              /* 0: exact mode, > 0: async mode */
    void* stream;
} lr_forward_args;

/*
 * lr_backward_args.  The outputs are lr_backward's; in raw mode they are gradients with respect to the stored tensors:
 * dL_dopacity = dL_dopacity_raw [P], dL_dmean3D = dL_dxyz [P,3], dL_dsh = dL_dfeatures_dc [P,3], dL_dsh_rest = dL_dfeatures_rest
 * [P,M-1,3] (required iff M > 1; NULL in activated mode), dL_dscale = dL_dscaling_raw [P,3], dL_drot = dL_drotation_raw [P,4],
 * dL_dmean2D [P,3] as in lr_backward; dL_dconic, dL_dcolor and dL_dcov3D are NULL.  accumulate_mask uses the LR_ACC_* bits of the
 * lr_backward outputs (LR_ACC_SH covers both feature tensors).
 *
 * Depth mode iff dL_depths and depth_image are both given: dL_depths [1,H,W] is HONOURED, with `depth_image` [1,H,W] the forward's
 * depth output (out_depth of the same view).  dL_depths without depth_image is LR_ERR_INVALID_ARG (lr_backward, the reference's
 * mirror, passes neither and so ignores its dL_depths); depth_image alone changes nothing (same kernels, same bits).
 * The derivative is that of what the forward outputs, depth = D / acc where acc > 0.5 and 0 elsewhere, with
 * D = sum z_i w_i, acc = 1e-6 + sum w_i, w_i = alpha_i T_i and z_i the view-space depth of Gaussian i; for an upstream g
 * and a pixel with depth != 0 (gz = g / acc, ga = -g depth / acc; pixels whose depth is 0 contribute nothing):
 *   - direct term: dL/dz_i += w_i gz, reaching dL/dmean3D (raw: dL/dxyz) through z = view[2] x + view[6] y + view[10] z + view[14];
 *   - through alpha: depth and coverage act as two more colour channels with values (z_i, 1), weights (gz, ga) and
 *     background 0, so dL/dmean2D, dL/dconic, dL/dopacity (and what follows from them) carry the depth loss's share --
 *     dL_dmean2D, which feeds densification, included.
 * The conventions of the colour path hold: the 0.99 clamp of alpha is not differentiated; the T < 1e-4 stop, the
 * alpha < 1/255 and power > 0 skips, the sort order and the acc > 0.5 mask are constants; the fov clamp is treated as there.
 * acc is taken as 1e-6 + (1 - final T) (equal to the forward's float sum up to rounding).  The blend backward walks every
 * tile's whole list in this mode (no list segments); no global float atomics: the result is bit-repeatable.  An async view
 * that overflowed its binning buffer writes nothing, as in lr_backward.
 *
 * Alpha mode iff dL_dalpha [1,H,W] is given: the gradient through the alpha output (lr_render_alpha) as well, alone or with depth
 * mode.  The derivative is that of 1 - prod_i (1 - alpha_i) over the layers the forward applied, with the colour path's conventions
 * (the 0.99 clamp of alpha not differentiated; the alpha < 1/255 and power > 0 skips, the T < 1e-4 stop -- whose trigger is not
 * applied -- and the sort order are constants; the fov clamp as there): d alpha_pix / d alpha_i = T_final / (1 - alpha_i).  It
 * reaches dL_dopacity, dL_dmean2D (which feeds densification), dL_dconic and through them means3D / xyz, scales, rotations and
 * cov3D; colours and SH get nothing from it.  Alone it runs the default backward's blend shape and list segments; with the depth
 * pair it joins the depth-mode kernel.  No global float atomics: bit-repeatable.
 *
 * Absgrad mode (AbsGS; gsplat's `absgrad`) iff dL_dmean2D_abs [P,3] is given (16-byte aligned; NULL simply means the mode is off --
 * the "dL_dmean2D_abs is required" check of the retired absgrad entries went with them).
 * Definition.  Let L be the scalar the call differentiates: sum dL_dpix . colour, plus the depth and alpha terms when their
 * gradients are given.  For pixel p and Gaussian i let g[p,i] in R^2 be the part of dL/dmeans2D_i[:2] that flows through pixel p,
 * in the NDC scale of dL_dmean2D (0.5 W, 0.5 H; backward.cu:473-474), so that sum_p g[p,i] = dL_dmean2D[i, :2].  Then
 *     dL_dmean2D_abs[i] = ( sum_p |g[p,i].x|,  sum_p |g[p,i].y|,  0 ).
 * Every convention of the signed path holds: the power > 0 and alpha < 1/255 skips, nothing behind a pixel's last contributor,
 * the 0.99 clamp not differentiated, strict mode (lr_tune_set("strict")) and anti-aliasing.  Rows with radii <= 0 are exact zeros.
 * dL_dmean2D_abs >= |dL_dmean2D| componentwise, with equality only where the per-pixel pulls do not cancel: a large Gaussian over
 * a blurry region has a near-zero signed gradient and a large absolute one, which is what a densification rule wants to see.
 * The tensor is always WRITTEN: zero-filled by the call (also under LR_ACC_NO_ZERO_FILL, like dL_dmean2D), never accumulated
 * (no bit of accumulate_mask refers to it), not part of the armed fused step.  Every other output is what the call without it
 * gives for the same arguments up to the rounding of another reduction order: the blend backward runs the 2-wave shape over
 * whole lists at every image size, as depth mode does.  No global float atomics: bit-repeatable.  lr_views_accumulate does not
 * hand out the tensor; it accumulates the norm of each view's into its densification statistics (stat_absgrad, below).
 */
typedef struct lr_backward_args {
    size_t struct_bytes;                     /* = sizeof(lr_backward_args); anything else is LR_ERR_INVALID_ARG */
    lr_view view;
    /* what the view's forward returned / wrote: num_rendered, radii [P] and the three scratch buffers */
    int R;
    const int* radii;
    char* geom_buffer;
    char* binning_buffer;
    char* image_buffer;
    /* upstream gradients: dL_dpix [3,H,W] required; the others select depth and alpha mode (see above) */
    const float* dL_dpix;
    const float* dL_depths;
    const float* depth_image;
    const float* dL_dalpha;
    /* gradient outputs (see above and lr_backward) */
    float* dL_dmean2D;
    float* dL_dmean2D_abs;
    float* dL_dconic;
    float* dL_dopacity;
    float* dL_dcolor;
    float* dL_dmean3D;
    float* dL_dcov3D;
    float* dL_dsh;
    float* dL_dsh_rest;
    float* dL_dscale;
    float* dL_drot;
    int debug;
    long long binning_capacity;              /* the value the forward was given */
    unsigned int accumulate_mask;
    void* stream;
} lr_backward_args;

/* Return values and errors are lr_forward's / lr_backward's.  A NULL pointer or a struct_bytes other than the struct's size is
 * LR_ERR_INVALID_ARG, checked before anything else. */
int lr_view_forward(const lr_forward_args* a);
int lr_view_backward(const lr_backward_args* a);

/*
 * Alpha output: the accumulated opacity alpha = 1 - T_final [1,H,W] of a forward, from its image buffer (the float32 T_final
 * the blend forward left there), written to out_alpha on `stream`.  0 where no Gaussian contributes.  Valid for activated and
 * raw forwards, exact and async mode: pass the image buffer of the forward whose colour you keep (after an overflow
 * re-render, the re-render's).  The forward's kernels are not changed by it.
 */
int lr_render_alpha(const char* image_buffer, int width, int height, float* out_alpha, void* stream);

/*
 * Median depth and per-pixel Gaussian ids of a forward, from its three scratch buffers; a pass of its own behind the forward,
 * whose kernels are not changed by it.
 *
 * Definition.  For one pixel, walk its tile's list front to back exactly as the blend forward does, T = 1 at the start:
 * power > 0 -> skip; alpha = min(0.99, opacity exp(power)), alpha < 1/255 -> skip; test_T = T (1 - alpha), test_T < 1e-4 -> stop,
 * not blended; otherwise blend, T = test_T.  The median Gaussian is the first blended Gaussian with test_T < 0.5: the layer at
 * which the transmittance first falls below one half.
 *   out_median_depth [1,H,W] float32: that Gaussian's view-space z, the per-Gaussian value the expected depth blends; 0 where T never
 *     falls below 0.5 (the depth output's "0 = no surface").  Unlike the expected depth D / acc it never lies between a foreground
 *     and a background surface.
 *   out_ids [H,W] int32, may be NULL: its row among the caller's P rows; -1 where there is none.
 * With the 0.99 clamp a pixel still at T >= 0.5 cannot trigger the 1e-4 stop (test_T >= 0.005): the two thresholds never interact.
 * The values hold under strict parity (lr_tune_set("strict"), which must be what the forward ran under), anti-aliasing, the 3D
 * filter, raw and activated parameters and both forward shapes: the pass evaluates alpha from the forward's records with the
 * forward's arithmetic in the forward's order, so its T sequence is the forward's bit for bit.
 * Valid for raw and activated forwards, exact and async mode (binning_capacity: the value the forward was given; the layout of
 * the binning buffer is resolved on the device), before or after the view's backward.  An async view that overflowed its binning
 * buffer writes 0 / -1 everywhere (rc 0; lr_check reports the overflow); so does a view without Gaussians, and P = 0 without
 * reading a buffer.  width x height must stay below 2^31.
 *
 * lr_median_backward: the gradient of out_median_depth.  The selection of the median Gaussian is a constant (as the sort order is
 * everywhere else): d median_depth[p] / d z_g = 1 for g = ids[p] and nothing else, reaching dL_dmean3D [P,3] (raw mode: dL/dxyz)
 * through z = view[2] x + view[6] y + view[10] z + view[14].  Nothing flows to opacity, covariance or colour: a weaker signal
 * than the expected depth's gradient (depth mode of lr_view_backward), enough to put lr_depth_l1_* / lr_depth_pearson_* on the
 * median depth.  ids: what lr_render_median wrote for the same buffers; radii: the forward's.  accumulate != 0: the rows of
 * Gaussians that own a tile instance are added to and every other row stays untouched; else dL_dmean3D is written in full,
 * rows with radii <= 0 as exact zeros.  An overflowed async view contributes nothing.  A gather per Gaussian in a fixed order,
 * no global float atomics: bit-repeatable.
 */
typedef struct lr_median_args {
    size_t struct_bytes;                     /* = sizeof(lr_median_args); anything else is LR_ERR_INVALID_ARG */
    const char* geom_buffer;
    const char* binning_buffer;
    const char* image_buffer;
    int P, width, height;
    long long binning_capacity;              /* the value the forward was given */
    float* out_median_depth;
    int* out_ids;                            /* may be NULL */
    void* stream;
} lr_median_args;

typedef struct lr_median_backward_args {
    size_t struct_bytes;                     /* = sizeof(lr_median_backward_args); anything else is LR_ERR_INVALID_ARG */
    const char* geom_buffer;
    const char* binning_buffer;
    const char* image_buffer;
    int P, width, height;
    long long binning_capacity;
    const int* radii;
    const int* ids;
    const float* dL_dmedian;
    const float* viewmatrix;
    float* dL_dmean3D;
    int accumulate;
    void* stream;
} lr_median_backward_args;

int lr_render_median(const lr_median_args* a);
int lr_median_backward(const lr_median_backward_args* a);

/*
 * Depth distortion of a forward (Mip-NeRF 360's distortion loss, as 2DGS and gsplat's `distloss` use it), from its three scratch
 * buffers; a pass of its own behind the forward, whose kernels are not changed by it.
 *
 * Definition.  For one pixel, walk its tile's list front to back exactly as the blend forward and lr_render_median do, T = 1 at the
 * start: power > 0 -> skip; alpha = min(0.99, opacity exp(power)), alpha < 1/255 -> skip; test_T = T (1 - alpha), test_T < 1e-4 ->
 * stop, not blended; otherwise the entry is blended with weight w_i = alpha_i T_i, then T = test_T.  Each blended layer has a mapped
 * depth m_i = map_c0 + map_c1 z_i + map_c2 / z_i, z_i the Gaussian's view-space depth (the per-Gaussian value the expected depth
 * blends).  Two mappings in use: 2DGS's far / (far - near) (1 - near / z), i.e. (c0, c1, c2) = (far / (far - near), 0,
 * -far near / (far - near)), and the linear one, (0, 1, 0).  The distortion of the pixel is
 *     D = sum_i w_i sum_{j<i} w_j (m_i - m_j)^2 = sum_i w_i (mt_i^2 A_{i-1} + M2_{i-1} - 2 mt_i M1_{i-1}),
 * A, M1, M2 the running sums of w, w mt and w mt^2, mt_i = m_i - m_ref, m_ref the mapped depth of the pixel's first blended layer
 * (D depends on differences only; the shift keeps the float32 moments from cancelling).
 *   out_distortion [1,H,W] float32: D >= 0; exactly 0 for a pixel with fewer than two blended layers.
 *   out_moments    [H,W,4] float32: {A, M1, M2, m_ref} per pixel, what lr_distortion_backward needs of this pass.
 * The values hold under strict parity (lr_tune_set("strict"), which must be what the forward ran under), anti-aliasing, the 3D
 * filter, raw and activated parameters and both forward shapes, as lr_render_median's do: the T sequence is the forward's bit for
 * bit.  Exact and async mode (binning_capacity: the value the forward was given); an async view that overflowed its binning buffer
 * writes zeros (rc 0; lr_check reports the overflow), as does P = 0, without reading a buffer.  width x height below 2^31.
 *
 * lr_distortion_backward: the gradient of out_distortion for the upstream dL_ddistortion [1,H,W], with `distortion` and `moments`
 * what lr_render_distortion wrote for the same buffers and the same three coefficients.  With g = dL/dD and the pixel's totals:
 *     q_i = dD/dw_i = mt_i^2 A - 2 mt_i M1 + M2,   dD/dm_i = 2 w_i (mt_i A - M1),
 *     dD/dalpha_i = T_i q_i - S_i / (1 - alpha_i),  S_i = sum_{k>i} w_k q_k = 2 D - sum_{k<=i} w_k q_k  (taken front to back).
 * The conventions of the colour path hold: the 0.99 clamp of alpha is not differentiated; the skips, the stop, the sort order and
 * m_ref are constants.  alpha = opacity G reaches dL_dmean2D, dL_dconic, dL_dopacity and through them the mean, scales, rotations
 * and cov3D; dL/dz_i = g dD/dm_i (map_c1 - map_c2 / z_i^2) reaches dL_dmean3D (raw: dL/dxyz) through the view matrix's z row.
 * Colours and SH get nothing: dL_dcolor, dL_dsh and dL_dsh_rest may be NULL and are never added to; given in write mode they are
 * zero-filled.  The other outputs, their units, accumulate_mask (LR_ACC_*, LR_ACC_NO_ZERO_FILL) and the alignment rule are
 * lr_backward_args'; `view` is the forward's (its shs / colors_precomp are not read).  Order: the per-tile kernel, the zero-fill of
 * rows in write mode, the depth-mode per-Gaussian backward.  The per-tile kernel OVERWRITES the per-instance gradient slots of the
 * binning buffer: the call runs after the colour backward (lr_view_backward) of the same forward state, on the same stream or
 * ordered behind it, and before another forward reuses the buffers.  An overflowed async view adds nothing.  No global float
 * atomics: bit-repeatable.  In lr_views_accumulate the term runs fused with the rendered normal map's (lr_geometry_backward).
 */
typedef struct lr_distortion_args {
    size_t struct_bytes;                     /* = sizeof(lr_distortion_args); anything else is LR_ERR_INVALID_ARG */
    const char* geom_buffer;
    const char* binning_buffer;
    const char* image_buffer;
    int P, width, height;
    long long binning_capacity;              /* the value the forward was given */
    float map_c0, map_c1, map_c2;            /* m = map_c0 + map_c1 z + map_c2 / z */
    float* out_distortion;
    float* out_moments;
    void* stream;
} lr_distortion_args;

typedef struct lr_distortion_backward_args {
    size_t struct_bytes;                     /* = sizeof(lr_distortion_backward_args); anything else is LR_ERR_INVALID_ARG */
    lr_view view;
    char* geom_buffer;
    char* binning_buffer;
    char* image_buffer;
    long long binning_capacity;
    const float* dL_ddistortion;
    const float* moments;
    const float* distortion;
    float map_c0, map_c1, map_c2;
    /* gradient outputs, as lr_backward_args */
    float* dL_dmean2D;
    float* dL_dconic;
    float* dL_dopacity;
    float* dL_dcolor;
    float* dL_dmean3D;
    float* dL_dcov3D;
    float* dL_dsh;
    float* dL_dsh_rest;
    float* dL_dscale;
    float* dL_drot;
    unsigned int accumulate_mask;
    void* stream;
} lr_distortion_backward_args;

int lr_render_distortion(const lr_distortion_args* a);
int lr_distortion_backward(const lr_distortion_backward_args* a);

/*
 * Rendered normal map of a forward (the "normal consistency" input of 2DGS section 5, RaDe-GS and PGSR: the per-pixel blend of the
 * Gaussians' normals, to be compared with the normals of the rendered depth), from its three scratch buffers; a pass of its own
 * behind the forward, whose kernels are not changed by it.
 *
 * Per-Gaussian normal.  Needs scales + rotations: with cov3D_precomp there is no normal and both entries return
 * LR_ERR_INVALID_ARG.
 *   Axis: k = argmin over the three scales; on ties the lowest index wins.  The comparison is made on the floats as given --
 *   activated scales, or in raw mode the stored log-scales -- an exact comparison of inputs.  scale_modifier, the 3D filter and
 *   anti-aliasing do not change k.  An isotropic Gaussian (LucidDreamer's freshly initialised ones are) takes axis 0.
 *   World space: n_world = R(q)[:, k], R the quaternion matrix for which Sigma = R S^2 R^T, so Sigma n = s_k^2 n.  Activated mode
 *   uses q as given, with no normalisation, as the covariance does; raw mode uses q / max(|q|, 1e-12).
 *   View space: n_view = W n_world, W the rotation part of the view matrix.  Axes: x right, y down, z forward (those of
 *   lr_depth_normals).
 *   Orientation: towards the camera (n . (u, v, 1) < 0, the depth normals' convention), decided once per Gaussian: with p_view the
 *   Gaussian's view-space mean, n_view . p_view > 0 -> n_view = -n_view.
 *   The axis choice and the sign are constants of the view, as the sort order is: nothing flows to scales or the mean through them.
 * Per-pixel map.  N = sum_i w_i n_i over the layers the blend forward applied to the pixel, w_i = alpha_i T_i with the forward's
 * skips, 0.99 clamp and 1e-4 stop: exactly the walk of lr_render_distortion.  No background term, no normalisation: |N| <= alpha,
 * and a caller divides by alpha or normalises as their method asks.
 *   out_normals       [3,H,W] float32: N; exact zeros for a pixel with no layer, for P = 0 and for an overflowed async view.
 *   out_gauss_normals [P,4]   float32: {n_view.xyz, sign (k + 1)} per Gaussian, zeros for radii <= 0; what
 *                                      lr_render_normals_backward needs of this pass.  16-byte aligned.
 * As for lr_render_distortion the definition holds under strict parity, anti-aliasing, the 3D filter, raw and activated
 * parameters, both forward shapes, and exact and async mode.  `view` is the forward's: scales, rotations, means3D, viewmatrix and
 * raw are read.  P = 0 returns 0 and writes zeros without reading a buffer.
 *
 * lr_render_normals_backward: the gradient of out_normals for the upstream dL_dnormals [3,H,W], with `normals` and `gauss_normals`
 * what lr_render_normals wrote for the same buffers.  With g = dL/dN of the pixel and c_i = n_i . g:
 *     dL/dn_i += w_i g,   dL/dalpha_i = T_i c_i - S_i / (1 - alpha_i),   S_i = sum_{k>i} w_k c_k = N.g - sum_{k<=i} w_k c_k,
 * S_i taken front to back on the forward's own T sequence.  The conventions of the colour path hold: the clamp is not
 * differentiated; skips, stop and order are constants.  alpha = opacity G reaches dL_dmean2D, dL_dconic and dL_dopacity and
 * through them the mean, scales and rotations.  dL/dn_i is summed per Gaussian into dL_dgauss_normal [P,3] (a public output,
 * written in full, 16-byte aligned) and goes on to dL_drot only: un-flip, W^T, the Jacobian of column k of R(q), and in raw mode
 * the normalisation Jacobian (g - q (q.g)) / |r|; it is ADDED to the rows of dL_drot with radii > 0.  Colours and SH get nothing:
 * dL_dcolor, dL_dsh and dL_dsh_rest may be NULL and are never added to; given in write mode they are zero-filled.  The other
 * outputs, their units, accumulate_mask and the alignment rule are lr_distortion_backward_args'.  Order: the per-tile kernel, the
 * zero-fill of rows in write mode, the per-Gaussian backward, the rotation chain.  The per-tile kernel OVERWRITES the per-instance
 * gradient slots of the binning buffer: the ordering rule is lr_distortion_backward's (behind the colour backward of the same
 * forward state -- and behind lr_distortion_backward, if both run -- and before another forward reuses the buffers).  An
 * overflowed async view adds nothing.  No global float atomics: bit-repeatable.  In lr_views_accumulate the term runs fused with
 * the distortion's (lr_geometry_backward).
 */
typedef struct lr_normals_render_args {
    size_t struct_bytes;                     /* = sizeof(lr_normals_render_args); anything else is LR_ERR_INVALID_ARG */
    lr_view view;
    const int* radii;                        /* the forward's [P] */
    const char* geom_buffer;
    const char* binning_buffer;
    const char* image_buffer;
    long long binning_capacity;              /* the value the forward was given */
    float* out_normals;
    float* out_gauss_normals;
    void* stream;
} lr_normals_render_args;

typedef struct lr_normals_render_backward_args {
    size_t struct_bytes;                     /* = sizeof(lr_normals_render_backward_args); anything else is LR_ERR_INVALID_ARG */
    lr_view view;
    char* geom_buffer;
    char* binning_buffer;
    char* image_buffer;
    long long binning_capacity;
    const float* dL_dnormals;
    const float* normals;
    const float* gauss_normals;
    const int* radii;
    float* dL_dgauss_normal;
    /* gradient outputs, as lr_backward_args */
    float* dL_dmean2D;
    float* dL_dconic;
    float* dL_dopacity;
    float* dL_dcolor;
    float* dL_dmean3D;
    float* dL_dcov3D;                        /* never written: there is no normal with cov3D_precomp */
    float* dL_dsh;
    float* dL_dsh_rest;
    float* dL_dscale;
    float* dL_drot;
    unsigned int accumulate_mask;
    void* stream;
} lr_normals_render_backward_args;

int lr_render_normals(const lr_normals_render_args* a);
int lr_render_normals_backward(const lr_normals_render_backward_args* a);

/*
 * N-channel feature map of a forward (semantic or instance logits, distilled 2D features as Feature-3DGS, LangSplat and
 * LEGaussians blend them, per-Gaussian appearance codes; gsplat renders any channel count), from its three scratch buffers; a
 * pass of its own behind the forward, whose kernels are not changed by it.
 *
 * Input.  features [P,C] float32, contiguous, 16-byte aligned, 1 <= C = `channels` <= LR_FEATURE_MAX_CHANNELS.  View-independent
 * and used as given in activated and in raw mode alike: there is no activation.
 * Per-pixel map.  F[c] = sum_i w_i f_i[c] over the layers the blend forward applied to the pixel, w_i = alpha_i T_i with the
 * forward's skips, 0.99 clamp and 1e-4 stop: exactly the walk of lr_render_normals and lr_render_distortion, the same T sequence.
 * No background term, no normalisation.
 *   out_features [C,H,W] float32, planar: F; exact zeros for a pixel with no layer, for P = 0 (no buffer is read) and for an
 *                                overflowed async view.
 * Every channel is an fma chain of its own in list order: a channel's bits do not depend on the other columns of `features` or
 * on C.  As for lr_render_normals the definition holds under strict parity, anti-aliasing, the 3D filter, raw and activated
 * parameters, both forward shapes, exact and async mode -- and with cov3D_precomp: nothing here needs scales or rotations.  Of
 * `view` the forward pass reads P, width and height only.
 *
 * lr_render_features_backward: the gradient of out_features for the upstream dL_dout_features [C,H,W], with `out_features` what
 * lr_render_features wrote for the same buffers and the same `features`.  With g = dL/dF of the pixel and c_i = f_i . g over all C
 * channels:
 *     dL/df_i[c] += w_i g[c],   dL/dalpha_i = T_i c_i - S_i / (1 - alpha_i),   S_i = sum_{k>i} w_k c_k = F.g - sum_{k<=i} w_k c_k,
 * S_i taken front to back on the forward's own T sequence, as lr_render_normals_backward takes it.  The conventions of the colour
 * path hold: the clamp is not differentiated; skips, stop and order are constants.  alpha = opacity G reaches dL_dmean2D,
 * dL_dconic and dL_dopacity with the expressions of the blend backward's flush, and through them the per-Gaussian backward, as it
 * stands and run ONCE per call, carries the gradient to the mean, scales and rotations (or cov3D: dL_dcov3D is written with
 * cov3D_precomp) and the opacity.
 *   dL_dfeatures [P,C] float32, 16-byte aligned: written in full in write mode -- rows with radii <= 0 and rows no pixel blended
 *   are exact zeros --, or with LR_ACC_FEATURES in accumulate_mask ADDED to in the rows of the Gaussians that own a tile instance
 *   (the others stay untouched).
 *   workspace: lr_features_workspace_bytes(slots, channels) device bytes, 16-byte aligned, `slots` the bound the binning buffer
 *   was laid out with or any bound above it: binning_capacity in async mode; in exact mode the value lr_forward returned (the
 *   reference's num_rendered is never below the instance count).  In async mode a workspace below the capacity's size is refused;
 *   in exact mode the host does not know the count: the kernels never touch a row outside the workspace, and a view with more
 *   instances than the workspace has rows is reported by lr_check as an incomplete backward.
 * Colours and SH get nothing: dL_dcolor, dL_dsh and dL_dsh_rest may be NULL and are never added to; given in write mode they are
 * zero-filled.  The other outputs, their units, accumulate_mask and the alignment rule are lr_distortion_backward_args'.  Order:
 * per chunk of channels the per-tile kernel and the per-Gaussian row sums of dL_dfeatures; then the zero-fill of rows in write
 * mode and the per-Gaussian backward.  The per-tile kernel OVERWRITES the per-instance gradient slots of the binning buffer: the
 * ordering rule is lr_normals_render_backward_args' (behind the colour backward of the same forward state -- and behind the other
 * passes' backwards, if they run -- and before another forward reuses the buffers).  An overflowed async view adds nothing.  No
 * global float atomics: two runs give the same bits, and a column of dL_dfeatures does not depend on the other channels.
 */
#define LR_FEATURE_MAX_CHANNELS 256
#define LR_ACC_FEATURES (1u << 9)            /* accumulate_mask of lr_render_features_backward: dL_dfeatures is added to */

typedef struct lr_feature_render_args {
    size_t struct_bytes;                     /* = sizeof(lr_feature_render_args); anything else is LR_ERR_INVALID_ARG */
    lr_view view;
    const int* radii;                        /* the forward's [P]; not read */
    const char* geom_buffer;
    const char* binning_buffer;
    const char* image_buffer;
    long long binning_capacity;              /* the value the forward was given */
    const float* features;                   /* [P,C] */
    int channels;
    float* out_features;                     /* [C,H,W] */
    void* stream;
} lr_feature_render_args;

typedef struct lr_feature_render_backward_args {
    size_t struct_bytes;                     /* = sizeof(lr_feature_render_backward_args); anything else is LR_ERR_INVALID_ARG */
    lr_view view;
    char* geom_buffer;
    char* binning_buffer;
    char* image_buffer;
    long long binning_capacity;
    const float* features;                   /* [P,C] */
    int channels;
    const float* dL_dout_features;           /* [C,H,W] */
    const float* out_features;               /* [C,H,W], for F.g */
    const int* radii;
    float* dL_dfeatures;                     /* [P,C] */
    void* workspace;
    size_t workspace_bytes;
    /* gradient outputs, as lr_backward_args */
    float* dL_dmean2D;
    float* dL_dconic;
    float* dL_dopacity;
    float* dL_dcolor;
    float* dL_dmean3D;
    float* dL_dcov3D;
    float* dL_dsh;
    float* dL_dsh_rest;
    float* dL_dscale;
    float* dL_drot;
    unsigned int accumulate_mask;
    void* stream;
} lr_feature_render_backward_args;

/* 0 for slots < 0 or channels outside 1 .. LR_FEATURE_MAX_CHANNELS; never decreasing in either argument otherwise */
size_t lr_features_workspace_bytes(long long slots, int channels);
int lr_render_features(const lr_feature_render_args* a);
int lr_render_features_backward(const lr_feature_render_backward_args* a);

/*
 * Depth distortion AND rendered normal map of a forward in ONE tile walk each way (render_geom.hip): the pair the multi-view
 * step runs for its two geometry regularisers.  The definitions are lr_render_distortion's and lr_render_normals', word for word
 * -- the mapped depth m = map_c0 + map_c1 z + map_c2 / z, the shift by m_ref, D >= 0, N = sum_i w_i n_i, the forward's skips, 0.99
 * clamp and 1e-4 stop; strict parity, anti-aliasing, the 3D filter, raw and activated parameters, both forward shapes, exact and
 * async mode; zeros for an overflowed async view and for P = 0 -- and every pixel is updated with the separate passes' expressions
 * in their order.  The argument structs are the unions of the two pairs' members.
 *
 * lr_render_geometry: the per-Gaussian normals first (out_gauss_normals [P,4], as lr_render_normals writes them), then one walk
 * that writes out_distortion [1,H,W], out_moments [H,W,4] and out_normals [3,H,W]; all four outputs are required (P = 0:
 * out_gauss_normals may be NULL).  cov3D_precomp has no normal: LR_ERR_INVALID_ARG.
 *
 * lr_geometry_backward: the gradient of both maps in one per-tile kernel and ONE per-Gaussian pass.  Upstreams: dL_ddistortion
 * [1,H,W] and dL_dnormals [3,H,W]; either may be NULL and then contributes nothing (both NULL: nothing is walked, the zero-fill
 * rule still holds).  With dL_ddistortion NULL, dL_ddistortion_scalar != 0 is the upstream of EVERY pixel (the step's weight x
 * mean(D) has weight / (H W) everywhere: it saves an image); with the image given the scalar is not read.  `distortion` and
 * `moments` are required with a distortion upstream, `normals` with dL_dnormals; gauss_normals, radii and dL_dgauss_normal [P,3]
 * (written in full) always.  Per blended layer the two dL/dalpha contributions are added per pixel before they are multiplied
 * out; the per-tile kernel leaves one GradRec per instance -- mean2D, conic, opacity, dL/dn in the colour floats, dL/dz in the free
 * float -- and the depth-mode per-Gaussian backward, as it stands, takes it on with dL_dgauss_normal in the colour row's place;
 * the rotation chain of lr_render_normals_backward follows.  The gradients agree with lr_distortion_backward +
 * lr_render_normals_backward on the same upstreams up to the rounding of the reduction order.  Outputs, units, accumulate_mask,
 * alignment: lr_normals_render_backward_args'.  The ordering rule is the same: behind the colour backward of the same forward
 * state, and before another forward reuses the buffers (the per-tile kernel OVERWRITES the per-instance gradient slots).  An
 * overflowed async view adds nothing.  No global float atomics: bit-repeatable.
 */
typedef struct lr_geometry_args {
    size_t struct_bytes;                     /* = sizeof(lr_geometry_args); anything else is LR_ERR_INVALID_ARG */
    lr_view view;                            /* the forward's: scales, rotations, means3D, viewmatrix, raw, P, width, height */
    const int* radii;                        /* the forward's [P] */
    const char* geom_buffer;
    const char* binning_buffer;
    const char* image_buffer;
    long long binning_capacity;              /* the value the forward was given */
    float map_c0, map_c1, map_c2;            /* m = map_c0 + map_c1 z + map_c2 / z */
    float* out_distortion;
    float* out_moments;
    float* out_normals;
    float* out_gauss_normals;
    void* stream;
} lr_geometry_args;

typedef struct lr_geometry_backward_args {
    size_t struct_bytes;                     /* = sizeof(lr_geometry_backward_args); anything else is LR_ERR_INVALID_ARG */
    lr_view view;
    char* geom_buffer;
    char* binning_buffer;
    char* image_buffer;
    long long binning_capacity;
    const float* dL_ddistortion;             /* [1,H,W] or NULL */
    float dL_ddistortion_scalar;             /* with dL_ddistortion NULL: dL/dD of every pixel (0: no distortion term) */
    const float* moments;
    const float* distortion;
    float map_c0, map_c1, map_c2;
    const float* dL_dnormals;                /* [3,H,W] or NULL */
    const float* normals;
    const float* gauss_normals;
    const int* radii;
    float* dL_dgauss_normal;
    /* gradient outputs, as lr_backward_args */
    float* dL_dmean2D;
    float* dL_dconic;
    float* dL_dopacity;
    float* dL_dcolor;
    float* dL_dmean3D;
    float* dL_dcov3D;                        /* never written: there is no normal with cov3D_precomp */
    float* dL_dsh;
    float* dL_dsh_rest;
    float* dL_dscale;
    float* dL_drot;
    unsigned int accumulate_mask;
    void* stream;
} lr_geometry_backward_args;

int lr_render_geometry(const lr_geometry_args* a);
int lr_geometry_backward(const lr_geometry_backward_args* a);

/*
 * Multi-view step (new; the reference renders one view per Python iteration, luciddreamer.py:291-304).
 * lr_views_accumulate runs lr_forward + the backward for n_views views of ONE parameter set and ACCUMULATES the gradients
 * into the acc_* buffers.  Everything is enqueued from C in one call: views alternate over up to 4 chains (forward of view
 * i+1 overlaps the backward of view i; the accumulating kernels are chained by events): the chain that ends with the last
 * view runs on `stream` itself, the others on streams of the library which are forked from / joined to `stream` with events
 * -- no host synchronisation; everything the call enqueued is ordered before whatever is enqueued on `stream` after it.
 * Async mode only (binning_capacity > 0); an overflow of any view is latched per slot and reported by lr_views_check (which
 * synchronises).  No config-level switch is read: which pointers are non-NULL selects the mode.
 *
 * Per-view arrays are HOST arrays of length n_views holding DEVICE pointers, or floats (tan_fovx, tan_fovy).  The driver of the
 * backward is EITHER fixed upstream gradients OR per-view targets (the fused training step); giving both is
 * LR_ERR_INVALID_ARG, as are depth_targets or masks without targets, and targets together with colors_precomp,
 * cov3D_precomp, acc_color or acc_cov3D.
 *   Fixed gradients: dL_dpix [3,H,W] per view, required.  dL_ddepth / dL_dalpha [H,W] per view, optional arrays: a view with
 *     a depth gradient runs the depth-mode backward of lr_view_backward fed with its own depth image, one with an alpha
 *     gradient its alpha-mode backward (depth + alpha with both), in the blend shape the view would
 *     take without it; a NULL entry gives that view the backward without that term.
 *   Fused training step (render -> loss -> backward per view, on the view's stream: the per-iteration body of the training
 *     loop, R/luciddreamer.py:296-304; gradients of sum_v loss_v; SH colours and scale/rotation covariances only):
 *     targets [3,H,W] per view, every entry required; loss = (1 - lambda_dssim) l1 + lambda_dssim (1 - ssim) as
 *       lr_l1_dssim_forward; out_losses (device, required) receives {loss, l1, ssim} per view.
 *     depth_targets [H,W] per view (optional array, no NULL entries; pixels whose target is not > 0, NaN included, are
 *       ignored) with depth_weight (finite, >= 0): loss += depth_weight * depth_l1, depth_l1 the unweighted masked mean of
 *       lr_depth_l1_forward; out_losses holds {loss, l1, ssim, depth_l1} per view.  With depth_weight == 0 the backward is the
 *       colour-only one (the bits of the step without depth_targets) and depth_l1 is still reported.
 *       depth_loss selects the depth term: LR_DEPTH_LOSS_L1 (0) the above, to the bit what the step computed before the member
 *       existed; LR_DEPTH_LOSS_PEARSON (1) the scale- and shift-invariant term of lr_depth_pearson_forward, loss += depth_weight *
 *       (1 - rho), with 1 - rho in the depth_l1 column of out_losses (same 4 or 5 columns) and the same depth_weight == 0 rule.
 *       A view whose term is degenerate (see there) reports 0 and gets a zero depth gradient: the colour-only gradients.  Any
 *       other value, or a non-zero value without depth_targets, is LR_ERR_INVALID_ARG.  Masks and the densification
 *       statistics compose with it unchanged.  It costs three launches per view where the L1 term has two.
 *     masks [H,W] in [0, 1] per view (optional array, no NULL entries; 1: content, 0: hole -- LucidDreamer's frames have holes:
 *       pixels the projected cloud left empty are exact zeros) with alpha_weight (finite, >= 0): the colour loss is that of the
 *       masked pair (lr_masked_l1_dssim_forward) and loss += alpha_weight * alpha_hole (lr_alpha_hole_forward on A = 1 -
 *       T_final of the view's forward); out_losses holds {loss, l1, ssim, depth_l1, alpha_hole} per view (depth_l1 = 0 without
 *       depth_targets, whose depth_weight is then ignored).  With alpha_weight == 0 the view gets no alpha gradient (for
 *       all-ones masks: the bits of the step without masks) and alpha_hole is still reported.
 *     distortion_weight / normal_consistency_weight (members of lr_views_geom_args, below; each finite and >= 0; they need
 *       targets, anything else is LR_ERR_INVALID_ARG): the two geometry regularisers.  A view of a step with a weight > 0 or with out_distortion /
 *       out_normals given runs lr_render_geometry behind its blend forward, on the view's stream, and
 *         loss += distortion_weight * mean(D),   D the depth distortion for distortion_map (c0, c1, c2),
 *         loss += normal_consistency_weight * sum_valid (1 - N . n) / (H W),   N the rendered normal map, n the normals of the
 *           view's rendered depth by lr_depth_normals' formula and validity rule (a pixel that is not valid adds nothing):
 *           the consistency term of lr_normal_loss_forward with N as target_normals, not normalised.
 *       out_losses then has SEVEN columns per view, {loss, l1, ssim, depth term, alpha_hole, distortion, normal_consistency}
 *       (mean(D) and the unweighted sum / (H W); absent terms 0); without the two terms it keeps its 3 / 4 / 5 columns.
 *       Backward: dL/dN = -weight n / (H W) on the valid pixels and the scalar weight / (H W) for dL/dD drive
 *       lr_geometry_backward behind the view's colour backward; its accumulation sits in the event chain that orders the views'.
 *       dL/ddepth of the normal term (through n) is added to the view's depth-gradient image: a step with
 *       normal_consistency_weight > 0 runs the depth-mode blend backward, with or without depth_targets.  A weight of 0 reports
 *       the term and leaves the gradients of the step without it, to the bit; with both weights 0 and no map asked for the pass
 *       does not run and the two columns are 0.  An overflowed view adds nothing and stays latched.
 *       The densification statistics (below) keep meaning the view's photometric / depth / alpha gradient: the geometry pass
 *       adds nothing to stat_grad_accum (with the normal term the depth part of G_v includes that term's dL/ddepth).
 * Workspace: lr_views_workspace_bytes(P, W, H, binning_capacity, n_streams, parts) device bytes, 256-byte aligned, with
 * `parts` the LR_VIEWS_* flags of what the step's slots hold besides a view's scratch: 0 for fixed gradients, LR_VIEWS_LOSS
 * with targets, | LR_VIEWS_DEPTH_LOSS with depth_targets, | LR_VIEWS_MASK_LOSS with masks (a mask step's slot always has the
 * depth part too: LOSS|MASK and LOSS|DEPTH|MASK are one layout), | LR_VIEWS_DEPTH_PEARSON with depth_loss ==
 * LR_DEPTH_LOSS_PEARSON (the slot's depth-loss workspace is then the larger one of lr_depth_pearson_workspace_bytes; valid only
 * together with LOSS and DEPTH or MASK; every other parts value keeps its sizes), | LR_VIEWS_GEOM when the step runs the geometry
 * pass (a weight > 0, or out_distortion / out_normals given; valid only together with LOSS; its part sits behind everything else in
 * a slot, so every parts value without it keeps its sizes).  DEPTH, MASK or GEOM without LOSS, or unknown bits, are invalid:
 * the size query returns 0 and lr_views_check LR_ERR_INVALID_ARG.  lr_views_check takes the values the step was run with.
 * Densification statistics (0.6.3): with stat_grad_accum, stat_denom and stat_max_radii [P] given -- all three or none, anything
 * else is LR_ERR_INVALID_ARG, as is stat_absgrad != 0 without them; 4-byte aligned, accumulated into, no accumulate-mask bit
 * refers to them, no extra workspace -- the call leaves them as if, for every view v of the step in order,
 *     lr_densify_stats(P, radii_v, G_v, stat_grad_accum, stat_denom, stat_max_radii)
 * had run with the view's own gradient G_v, which the step never materialises: per Gaussian with radii_v > 0,
 * stat_grad_accum += |G_v.xy|, stat_denom += 1, stat_max_radii = max(stat_max_radii, radii_v) -- the reference's rule, the norm
 * PER VIEW and then the sum (R/scene/gaussian_model.py:405-407), which acc_mean2D (the signed sum over the views) cannot give.
 *   stat_absgrad == 0: G_v is the dL_dmean2D lr_view_backward would write for that view alone, with every term the view has in
 *     the step (colour, depth, alpha; fixed gradients or fused loss).  The step's other outputs keep their bits.
 *   stat_absgrad != 0: G_v is that call's dL_dmean2D_abs (Absgrad mode above); as there, every view's blend backward then runs
 *     the absgrad kernel shape and the step's gradients agree with the step without it up to the rounding of the reduction order.
 * The visibility rule is radii_v > 0, not "owns a tile instance": a Gaussian whose tiles were all culled still counts in
 * stat_denom and stat_max_radii, with a norm of 0.  A view that overflowed its binning buffer contributes nothing to the three
 * tensors, as its backward writes nothing (the overflow stays latched for lr_views_check).  No global float atomics: the
 * accumulations are chained in view order, so the statistics are bit-repeatable and the same bits for every n_streams.
 * stat_denom and stat_max_radii equal the per-view route exactly, stat_grad_accum up to float rounding (the sum over the step's
 * views is formed first, then added).
 * (The positional lr_views_* entry points of library versions up to 0.5, one family per mode, are gone.)
 */
#define LR_VIEWS_LOSS        1u   /* slot holds the colour-loss workspace and dL/dcolor image   */
#define LR_VIEWS_DEPTH_LOSS  2u   /* ... and the depth gradient image + depth-L1 workspace      */
#define LR_VIEWS_MASK_LOSS   4u   /* ... and the alpha gradient image + alpha-hole workspace    */
#define LR_VIEWS_DEPTH_PEARSON 16u /* the depth-loss workspace holds the Pearson term's (8u is not a flag) */
#define LR_VIEWS_GEOM        64u  /* ... and the geometry pass's maps, upstream images and workspace (32u is not a flag) */

/* lr_views_args::depth_loss */
#define LR_DEPTH_LOSS_L1      0   /* masked depth L1 (lr_depth_l1_*) */
#define LR_DEPTH_LOSS_PEARSON 1   /* 1 - Pearson correlation (lr_depth_pearson_*) */

typedef struct lr_views_args {
    size_t struct_bytes;                     /* = sizeof(lr_views_args) (as lr_views_geom_args::base: of that struct) */
    /* the views: n_views and per-view camera data (all required) */
    int n_views;
    const float* const* viewmatrices;
    const float* const* projmatrices;
    const float* const* cam_positions;
    const float* tan_fovx;
    const float* tan_fovy;
    /* the scene, as in lr_forward (shs or colors_precomp; scales + rotations or cov3D_precomp) */
    int P, D, M;
    const float* background;
    int width, height;
    const float* means3D;
    const float* shs;
    const float* colors_precomp;
    const float* opacities;
    const float* scales;
    const float* rotations;
    const float* cov3D_precomp;
    float scale_modifier;
    /* fixed upstream gradients per view (see above) */
    const float* const* dL_dpix;
    const float* const* dL_ddepth;
    const float* const* dL_dalpha;
    /* the fused training step (see above); out_losses: device float[(3, 4 or 5) * n_views] */
    const float* const* targets;
    float lambda_dssim;
    const float* const* depth_targets;
    float depth_weight;
    const float* const* masks;
    float alpha_weight;
    float* out_losses;
    /* optional per-view outputs, fully written: colour [3,H,W], depth [H,W], alpha A = 1 - T_final [H,W] (lr_render_alpha's
     * values), radii [P]; NULL entries or arrays: not returned (a view whose depth is neither returned nor read by the step --
     * depth_targets, dL_ddepth -- is blended without the depth channel: same colour, alpha, radii and gradients to the bit).
     * out_color: a NULL entry (or array) means that the view's colour is formed only where the step itself reads it -- the losses
     * of a step with targets, and a view that carries its depth.  A depth-free view of a step driven by fixed upstream gradients
     * blends no colour at all: the backward starts from T_final and the last contributor, so alpha, radii and gradients are the
     * same bits; a view whose out_color entry is given gets its image as ever, and mixed steps are legal. */
    float* const* out_color;
    float* const* out_depth;
    float* const* out_alpha;
    int* const* out_radii;
    /* the accumulators, shaped like lr_backward's outputs; acc_mean2D, acc_opacity and acc_mean3D are required, the others
     * may be NULL when the corresponding input is absent */
    float* acc_mean2D;
    float* acc_opacity;
    float* acc_color;
    float* acc_mean3D;
    float* acc_cov3D;
    float* acc_sh;
    float* acc_scale;
    float* acc_rot;
    /* densification statistics (see above): all three or none; accumulated into */
    float* stat_grad_accum;                  /* [P] (a [P,1] tensor as is) */
    float* stat_denom;                       /* [P] */
    float* stat_max_radii;                   /* [P] */
    int    stat_absgrad;                     /* 0: norm of the signed per-view gradient; != 0: of the absolute one */
    /* workspace (lr_views_workspace_bytes for the same P, width, height, binning_capacity, n_streams and the step's parts),
     * number of chains (clamped to 1..4) and the caller's HIP stream */
    char* workspace;
    size_t workspace_bytes;
    long long binning_capacity;
    int n_streams;
    void* stream;
    /* the depth term of the fused training step (LR_DEPTH_LOSS_*; see above).  The LAST member on purpose: sizeof grows with
     * it, so a caller built against the header without it is rejected by the struct_bytes check instead of having whatever
     * sat in a padding hole read as a mode */
    int depth_loss;
} lr_views_args;

/*
 * lr_views_args with the two geometry regularisers of the fused training step (see above).  Their members lie behind depth_loss,
 * for the reason given there: `base` is the first member, so they follow everything lr_views_args holds, the struct has another
 * sizeof, and lr_views_args itself keeps its layout, with depth_loss as its last member.  A step with the terms passes
 * &args.base to lr_views_accumulate with base.struct_bytes = sizeof(lr_views_geom_args); struct_bytes = sizeof(lr_views_args)
 * is the step without them.  All zero / NULL: that step, to the bit.
 */
typedef struct lr_views_geom_args {
    lr_views_args base;                      /* base.struct_bytes = sizeof(lr_views_geom_args) */
    float distortion_weight;                 /* finite, >= 0 */
    float distortion_map[3];                 /* c0, c1, c2 of m = c0 + c1 z + c2 / z; read when the distortion is formed */
    float normal_consistency_weight;         /* finite, >= 0 */
    float* const* out_distortion;            /* optional per-view outputs [1,H,W] / [3,H,W], under out_depth's NULL rules */
    float* const* out_normals;
} lr_views_geom_args;

/* a->struct_bytes: sizeof(lr_views_args), or sizeof(lr_views_geom_args) for the base of one; anything else is LR_ERR_INVALID_ARG */
int lr_views_accumulate(const lr_views_args* a);
size_t lr_views_workspace_bytes(int P, int width, int height, long long binning_capacity, int n_streams, unsigned parts);
int lr_views_check(const char* workspace, int P, int width, int height, long long binning_capacity, int n_streams,
                   unsigned parts, void* stream);

/*
 * Row surgery of the Gaussian parameter set.  The reference changes the number of Gaussians
 * with boolean-mask indexing / torch.cat applied tensor by tensor to the six parameters and both Adam moments of
 * each (R/scene/gaussian_model.py:273-340 prune_points, _prune_optimizer, cat_tensors_to_optimizer; :342-403
 * densify_and_clone / densify_and_split / densify_and_prune).
 *   lr_select_rows: for every i in [0,P) with mask[i] != 0, in increasing i, row i of each of the n_tensors source
 *     tensors is copied to row (dst_row_offset + rank(i)) of its destination; rank(i) = number of selected rows
 *     before i.  row_bytes[t] (multiple of 4) is the row size of tensor t; src/dst/row_bytes are HOST arrays of
 *     n_tensors (<= 32) entries holding DEVICE pointers; dst may alias src only when dst_row_offset >= P (appending
 *     behind the live rows of a capacity buffer); a compaction goes to the other half of a ping-pong buffer.  *out_count (device int) receives the number
 *     of selected rows.  n_tensors == 0 only counts.  No host synchronisation.
 *   lr_pack_ply_rows: builds the 17 + 3*(M-1) float vertex records written by GaussianModel.save_ply (:193-208:
 *     x y z nx ny nz, f_dc_*, f_rest_* channel-major, opacity, scale_*, rot_*) in out_rows [P, 17+3(M-1)] (device).
 */
/* Densification statistics of one rendered view in one pass (R/luciddreamer.py:310-311 and R/scene/gaussian_model.py:405-407):
 * for every Gaussian with radii > 0: max_radii2D = max(max_radii2D, radii); xyz_gradient_accum += |dL_dmean2D[:, :2]|;
 * denom += 1.  radii [P] int32, dL_dmean2D [P,3] (the gradient of `means2D`), statistics [P,1], [P,1], [P] float32. */
int lr_densify_stats(int P, const int* radii, const float* dL_dmean2D, float* xyz_gradient_accum, float* denom,
                     float* max_radii2D, void* stream);
size_t lr_select_workspace_bytes(int P);
int lr_select_rows(int P, const unsigned char* mask, int n_tensors, const void* const* src, void* const* dst,
                   const unsigned* row_bytes, long long dst_row_offset, int* out_count, void* workspace,
                   size_t workspace_bytes, void* stream);
int lr_pack_ply_rows(int P, int M, const float* xyz, const float* features_dc, const float* features_rest,
                     const float* opacity, const float* scaling, const float* rotation, float* out_rows, void* stream);

/*
 * One-launch Adam step over the parameter tensors of a GaussianModel (the optimiser step after the gradient
 * all-reduce of the data-parallel step; the reference uses torch.optim.Adam(l, lr=0.0, eps=1e-15) with one param group
 * -- one learning rate -- per tensor, R/scene/gaussian_model.py:152-165).  Formula and operation order of torch's
 * single-tensor Adam without weight decay / amsgrad / maximize.  params, grads, exp_avg, exp_avg_sq, numel, lr are
 * HOST arrays of n_tensors (<= 16) entries (device pointers / element counts / learning rates); step is the 1-based
 * step count of these tensors.  Hyper-parameters are doubles (as in Python) and rounded to float once, after
 * 1 - beta and lr / (1 - beta1^t) have been formed.  Updates params, exp_avg, exp_avg_sq in place.
 */
int lr_adam_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                 float* const* exp_avg_sq, const unsigned long long* numel, const double* lr, double beta1, double beta2,
                 double eps, int step, void* stream);

/*
 * lr_adam_step for gradients that are only VALID in the rows of the Gaussians one view visited (SURVEY.md section 8f-4;
 * R/luciddreamer.py:296-327 runs `loss.backward()` and `optimizer.step()` back to back, one view per iteration).  A backward
 * called with LR_ACC_NO_ZERO_FILL in its accumulate_mask writes the gradient rows of the Gaussians that own a tile instance and
 * leaves every other row of its write-mode outputs UNWRITTEN (dL_dmean2D excepted, which is zero-filled as always: its readers
 * go by radii > 0); this step takes the gradient of a Gaussian without a tile instance as zero without reading it -- or of every
 * Gaussian, when the view overflowed its binning buffer and the backward skipped it.  Saved against lr_backward* +
 * lr_adam_step: the zero-fill pass over the gradient tensors (the reference memsets 300 B per Gaussian per backward,
 * rasterize_points.cu:154-162) and the read of those zeros.  Same arithmetic element for element: parameters and moments are
 * bit-identical to the unmasked pair.  geom_buffer: the scratch of the view's forward (its per-Gaussian instance counts are the
 * mask); every tensor must have P rows, row_len[t] floats each (numel[t] = P * row_len[t]), all arrays 16-byte aligned.
 */
int lr_adam_step_masked(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                        float* const* exp_avg_sq, const unsigned long long* numel, const unsigned int* row_len, const double* lr,
                        double beta1, double beta2, double eps, int step, const char* geom_buffer, int P, void* stream);

/*
 * MCMC densification (Kheradmand et al., "3D Gaussian Splatting as Markov Chain Monte Carlo", 2024): the per-row work of a
 * strategy with a fixed budget of Gaussians -- dead ones are relocated onto live ones, the set grows by a fixed rate up to a cap,
 * and a small position noise is added after every optimizer step (luciddreamer_amd/mcmc.py drives it).
 * All tensors are the STORED GaussianModel parameters: xyz [P,3], features_dc [P,1,3], features_rest [P,M-1,3], logit opacity
 * [P,1], log scaling [P,3], unnormalised rotation quaternion [P,4] in (r,x,y,z) order; float32, contiguous, device.
 *
 *   lr_mcmc_relocate: n pairs (dst[j], src[j]), device int32.  With c[i] the number of j with src[j] == i and
 *     N_i = min(c[i] + 1, n_max), every source i with c[i] > 0 -- o = sigmoid(opacity[i]) clamped to at most 1 - 2^-24 and
 *     s = exp(scaling[i]), both the values BEFORE the call -- gets
 *         o' = 1 - (1 - o)^(1/N_i)                                        (evaluated as -expm1(log1p(-o) / N_i))
 *         s' = s o / den,  den = sum_{m=1..N_i} sum_{k=0..m-1} C(m-1,k) (-1)^k / sqrt(k+1) o'^(k+1)    (in double)
 *     and logit(clamp(o', min_opacity, 1 - 1.1920929e-7)) and log(s') are stored in row i and in every dst[j] with src[j] == i;
 *     each such dst[j] also receives row i's xyz, features_dc, features_rest and rotation unchanged.  Both Adam moments of all
 *     six tensors (exp_avg / exp_avg_sq, in the order xyz, features_dc, features_rest, opacity, scaling, rotation; a NULL entry
 *     means there is no such tensor) are set to zero at every touched source row AND every destination row: a destination's
 *     moments belong to a Gaussian that no longer exists.  Rows that are neither are left bit-identical.  Deterministic: the
 *     only atomics are integer counts, and the result is bit-repeatable.
 *     The caller guarantees what the library cannot see without reading the device: {dst} and {src} are disjoint, dst has no
 *     duplicates (src may repeat), and every index is in [0, P_rows) -- P_rows is the number of rows the tensors can address,
 *     so for growth dst may lie behind the live rows of a capacity buffer.  Checked on the host (LR_ERR_INVALID_ARG): struct_bytes,
 *     n >= 0, P_rows >= 1, M >= 1, n_max in [1, 51], the index arrays, the six parameters (features_rest only for M > 1) and
 *     a workspace of lr_mcmc_workspace_bytes(P_rows, n) bytes.  n == 0 succeeds and launches nothing.  No host synchronisation.
 *   lr_mcmc_noise: xyz[i] += Sigma_i xi_i g(o_i) scaler, Sigma = R diag(s^2) R^T with R the rotation of the normalised
 *     quaternion (the covariance the preprocess builds, no scale modifier), xi = noise [P,3] standard-normal draws and
 *     g(o) = 1 / (1 + exp(-100 ((1 - o) - 0.995))), which leaves all but nearly transparent Gaussians where they are.
 *     56 bytes read and 12 written per Gaussian.
 *   lr_mcmc_reg_grad: adds the gradient of opacity_reg * mean(sigmoid(opacity)) + scale_reg * mean(exp(scaling)) to existing
 *     gradient buffers: dL_dopacity[i] += opacity_reg / P * o (1 - o), dL_dscale[i,c] += scale_reg / (3 P) * exp(scaling[i,c]).
 */
typedef struct lr_mcmc_relocate_args {
    size_t struct_bytes;                     /* = sizeof(lr_mcmc_relocate_args); anything else is LR_ERR_INVALID_ARG */
    int n;                                   /* number of pairs */
    const int* dst;                          /* [n] device: rows that are overwritten */
    const int* src;                          /* [n] device: rows they become copies of */
    int P_rows;                              /* rows the tensors can address (every index is below it) */
    int M;                                   /* SH coefficients per Gaussian: features_rest has M - 1 rows of three */
    float* xyz;
    float* features_dc;
    float* features_rest;                    /* NULL when M == 1 */
    float* opacity;
    float* scaling;
    float* rotation;
    float* exp_avg[6];                       /* xyz, features_dc, features_rest, opacity, scaling, rotation; NULL = none */
    float* exp_avg_sq[6];
    float min_opacity;                       /* lower clamp of the new opacities */
    int n_max;                               /* cap of N_i, 1..51 (51: the published implementations' table size) */
    void* workspace;                         /* lr_mcmc_workspace_bytes(P_rows, n) device bytes, 256-byte aligned */
    size_t workspace_bytes;
    void* stream;
} lr_mcmc_relocate_args;

int lr_mcmc_relocate(const lr_mcmc_relocate_args* a);
size_t lr_mcmc_workspace_bytes(int P_rows, int n);
int lr_mcmc_noise(int P, float* xyz, const float* raw_scale, const float* raw_rotation, const float* raw_opacity,
                  const float* noise, float scaler, void* stream);
int lr_mcmc_reg_grad(int P, const float* raw_opacity, const float* raw_scale, float opacity_reg, float scale_reg,
                     float* dL_dopacity, float* dL_dscale, void* stream);

/*
 * 3D smoothing filter (Yu et al., "Mip-Splatting: Alias-free 3D Gaussian Splatting", 2024): the half of Mip-Splatting that acts
 * on the Gaussians themselves; the other half, the 2D Mip filter, is lr_set_antialiasing, and the two are independent.  Every
 * Gaussian is convolved with an isotropic low-pass whose size follows the highest sampling rate at which any training camera
 * sees it (luciddreamer_amd/filter3d.py drives it).  All tensors float32, contiguous, device.
 *
 *   lr_filter3d_update: cams [V,20] = per camera the 16 floats of world_view_transform M in the row-vector convention the
 *     rasterizer uses ([x y z 1] M), then fx = W / (2 tan(FoVx / 2)), fy = H / (2 tan(FoVy / 2)), W, H.  With (x, y, z) the
 *     view-space position, formed as ((M[0][j] px + M[1][j] py) + M[2][j] pz) + M[3][j], camera n SEES Gaussian k iff
 *         z > 0.2   and   |x / z * fx| <= 0.65 W   and   |y / z * fy| <= 0.65 H
 *     (the near cull of the rasterizer; the image extended by 15 % on every side).  All of it in float32, one rounding per
 *     operation, no fused multiply-add.  Then
 *         d_k = min over the cameras that see k of z / fx        (the reciprocal of the paper's maximal sampling rate)
 *         filter3D[k] = sqrt(variance) d_k                       (variance: 0.2 in the paper)
 *     a Gaussian no camera sees gets sqrt(variance) max_k d_k over the seen ones, the widest filter in use, and if no Gaussian
 *     is seen at all (V == 0 included) every filter is 0 = no filtering.  seen [P] (one byte each, may be NULL) tells which.
 *     This is the paper's definition; its released code takes min z and max focal length separately, which is the same when
 *     all cameras share a focal length and a smaller filter otherwise.  Two launches, min and max only: bit-repeatable.
 *     workspace: lr_filter3d_workspace_bytes(P) device bytes.
 *   lr_filter3d_apply_forward: r_j = raw_scale[k][j] (log scale), q = raw_opacity[k] (logit), f = filter3D[k]:
 *         t_j = f^2 exp(-2 r_j),   h_j = log1p(t_j) / 2    (for t_j > 1: log f - r_j + log1p(1 / t_j) / 2, finite for tiny scales)
 *         log s'_j = r_j + h_j           so that s'_j = sqrt(s_j^2 + f^2)
 *         log c = -(h_0 + h_1 + h_2)     so that c = sqrt(prod s_j^2 / prod (s_j^2 + f^2))
 *         o' = sigmoid(q) c
 *     activated != 0: out_scale = s' = exp(log s'), out_opacity = o'   (what a rasterizer fed with activated values takes)
 *     activated == 0: out_scale = log s', out_opacity = logit(o') = log sigmoid(q) + log c - log(1 - o'), with
 *                     1 - o' = sigmoid(-q) + sigmoid(q) (-expm1(log c))   (what every raw-parameter path and a .ply take)
 *     A row with f <= 0 is not filtered: in the stored domain it keeps its bits.
 *   lr_filter3d_apply_backward: the gradient of the above with respect to raw_scale and raw_opacity (the filter is a constant),
 *     recomputed from the inputs; dL_dscale_out [P,3] / dL_dopacity_out [P] are the upstream gradients, NULL = zero.  With
 *     u_j = 1 / (1 + t_j), w_j = 1 - u_j (both formed without a subtraction):
 *         activated: dL/dr_j = g_j s'_j u_j + g_o o' w_j              dL/dq = g_o c sigmoid(q) sigmoid(-q)
 *         stored   : dL/dr_j = g_j u_j + g_o w_j / (1 - o')           dL/dq = g_o sigmoid(-q) / (1 - o')
 *     Both outputs are written in full.
 * 36 bytes per Gaussian forward, 52 backward.  P == 0 succeeds and launches nothing.  No host synchronisation.  Checked on the
 * host (LR_ERR_INVALID_ARG): P, V >= 0, variance finite and >= 0, the required pointers.
 */
size_t lr_filter3d_workspace_bytes(int P);
int lr_filter3d_update(int P, int V, const float* means3D, const float* cams, float variance, float* filter3D,
                       unsigned char* seen, char* workspace, void* stream);
int lr_filter3d_apply_forward(int P, const float* raw_scale, const float* raw_opacity, const float* filter3D, int activated,
                              float* out_scale, float* out_opacity, void* stream);
int lr_filter3d_apply_backward(int P, const float* raw_scale, const float* raw_opacity, const float* filter3D, int activated,
                               const float* dL_dscale_out, const float* dL_dopacity_out, float* dL_draw_scale,
                               float* dL_draw_opacity, void* stream);

/*
 * Fused photometric loss of the training loop:
 *     loss = (1 - lambda) * mean|image - gt| + lambda * (1 - mean(SSIM_map(image, gt)))
 * replacing l1_loss + ssim of R/utils/loss.py:18-69 as composed in R/luciddreamer.py:301-304 (11x11 window = outer
 * product of a normalised Gaussian, sigma 1.5; zero padding 5; C1 = 0.01^2, C2 = 0.03^2; mean over all C*H*W).
 * image, gt: [C,H,W] float32, contiguous (a batch [B,C,H,W] is passed as channels = B*C).
 *   lr_l1_dssim_forward : out_loss3 (device, 3 floats) = {loss, l1, ssim}; fills `workspace` (device,
 *                         lr_loss_workspace_bytes) with what the backward needs.  No host synchronisation.
 *   lr_l1_dssim_backward: dL_dimage [C,H,W] = upstream * d loss / d image, from the workspace of the forward on the
 *                         same inputs; `upstream` is a device scalar (autograd's grad_output) or NULL for 1.
 * Deterministic (no atomics).  Return 0 or a negative LR_ERR_*.
 */
size_t lr_loss_workspace_bytes(int channels, int height, int width);
int lr_l1_dssim_forward(int channels, int height, int width, const float* image, const float* gt, float lambda_dssim,
                        float* out_loss3, void* workspace, size_t workspace_bytes, void* stream);
int lr_l1_dssim_backward(int channels, int height, int width, const float* image, const float* gt, float lambda_dssim,
                         const float* upstream, const void* workspace, float* dL_dimage, void* stream);
/* The same backward for a caller that composes l1 and ssim ITSELF (R/luciddreamer.py:301-303 calls l1_loss and ssim
 * separately and weights them in Python): dL_dimage = w_l1[0] * d l1 / d image + w_ssim[0] * d ssim / d image, both weights
 * device scalars (autograd's grad_outputs of the two means) -- no host synchronisation to read them. */
int lr_l1_dssim_backward_weights(int channels, int height, int width, const float* image, const float* gt, const float* w_l1,
                                 const float* w_ssim, const void* workspace, float* dL_dimage, void* stream);

/*
 * Masked depth L1, for supervising the rendered depth with a depth map (e.g. a monocular estimate):
 *     loss = weight * mean_{H*W}( |depth - target| * [target > 0] )
 *     d loss / d depth = weight * sign(depth - target) * [target > 0] / (H*W)      (sign(0) = 0)
 * depth, target: [H,W] float32 device images, contiguous (a [1,H,W] depth output as is).  Pixels whose target is not > 0
 * (no estimate, NaN) contribute nothing, to the value and to the gradient.
 *   lr_depth_l1_forward : out_loss (device, 1 float); fills `workspace` (device, lr_depth_l1_workspace_bytes) with
 *                         per-workgroup partial sums, reduced in a fixed order in double.  No host synchronisation.
 *   lr_depth_l1_backward: dL_ddepth [H,W] = upstream * d loss / d depth; `upstream` is a device scalar (autograd's
 *                         grad_output) or NULL for 1.  The gradient does not depend on the loss value: one elementwise pass,
 *                         no workspace.
 * Deterministic (no atomics): the value is bit-repeatable.  Return 0 or a negative LR_ERR_*.
 */
size_t lr_depth_l1_workspace_bytes(int height, int width);
int lr_depth_l1_forward(int height, int width, const float* depth, const float* target, float weight, float* out_loss,
                        void* workspace, size_t workspace_bytes, void* stream);
int lr_depth_l1_backward(int height, int width, const float* depth, const float* target, float weight, const float* upstream,
                         float* dL_ddepth, void* stream);

/*
 * Pearson depth loss: scale- and shift-invariant supervision of the rendered depth by an ESTIMATED depth map (a monocular
 * estimate is right about ordering and relative structure, wrong about scale and offset, differently in every frame; the
 * correlation is invariant to target -> a * target + b, a > 0).  depth, target: [H,W] float32 device images, contiguous.
 * The valid set is M = {i : target_i > 0}, exactly lr_depth_l1_*'s: NaN targets and targets <= 0 are excluded, selected away,
 * never multiplied; m = |M|.  All sums run over M, in double:
 *     Sd = sum d, St = sum t, Sdd = sum d^2, Stt = sum t^2, Sdt = sum d t
 *     mu_d = Sd / m, mu_t = St / m
 *     Sxx = Sdd - Sd^2 / m, Syy = Stt - St^2 / m, Sxy = Sdt - Sd St / m
 *     rho = Sxy / sqrt(Sxx Syy), clamped to [-1, 1]
 *     term = 1 - rho, loss = weight * term
 *     for i in M: d loss / d d_i = -weight * ( (t_i - mu_t) / sqrt(Sxx Syy) - rho (d_i - mu_d) / Sxx ), and 0 outside M
 * Degenerate inputs -- m < 2, Sxx <= 1e-12 Sdd or Syy <= 1e-12 Stt (sums that are not finite count as such) -- have no
 * correlation: term = 0, loss = 0, rho = 0 and the gradient is exactly zero everywhere; no NaN or Inf reaches an accumulator.
 * (1e-12 is four orders of magnitude above the double-precision cancellation error of the one-pass variance.)
 * Every pixel's d and t are converted to double before any product or sum is formed; per-lane, per-workgroup and final sums are
 * double, in a fixed order, no atomics: the value is bit-repeatable from call to call.
 *   lr_depth_pearson_forward : out (device, 2 floats) = {loss, rho}; fills `workspace` (device, lr_depth_pearson_workspace_bytes:
 *                              six partial sums per workgroup and, behind them, a coefficient record -- mu_d, mu_t,
 *                              1 / sqrt(Sxx Syy), rho / Sxx, both 0 when degenerate).  weight finite and >= 0.
 *   lr_depth_pearson_backward: dL_ddepth [H,W] = upstream * d loss / d depth; `upstream` a device scalar or NULL for 1.  UNLIKE
 *                              lr_depth_l1_backward it READS the coefficient record the forward left in `workspace`: pass the same
 *                              workspace, untouched since the forward of the same depth, target, on the same stream (or ordered
 *                              behind it).  One elementwise pass.
 * No host synchronisation.  Return 0 or a negative LR_ERR_*; the argument checks (NULL pointers, sizes, workspace_bytes, weight)
 * precede every device call.
 */
size_t lr_depth_pearson_workspace_bytes(int height, int width);
int lr_depth_pearson_forward(int height, int width, const float* depth, const float* target, float weight, float* out,
                             void* workspace, size_t workspace_bytes, void* stream);
int lr_depth_pearson_backward(int height, int width, const float* depth, const float* target, float weight, const float* upstream,
                              const void* workspace, size_t workspace_bytes, float* dL_ddepth, void* stream);

/*
 * Mask supervision of one view (the single-view building blocks of lr_views_accumulate with masks).  mask: [H,W] float32
 * device image in [0, 1], 1 where the target frame has content, 0 in its holes; shared by the channels of image / gt.
 *   lr_masked_l1_dssim_forward / _backward: lr_l1_dssim_forward / _backward of the masked pair (mask * image, mask * gt) --
 *     loss = l1_dssim(m I, m G, lambda), dL_dimage = upstream * m * (d l1_dssim / dI')|_{I' = m I} -- with the same workspace
 *     (lr_loss_workspace_bytes), window, zero padding and mean over C*H*W.  Every product by m is exact for m == 1: an all-ones
 *     mask gives the bits of lr_l1_dssim_*.
 *   lr_alpha_hole_forward : out_loss (device, 1 float) = weight * mean_{H*W}( alpha * (1 - mask) ), alpha [H,W] (1 - T_final,
 *                           e.g. lr_render_alpha's output); per-workgroup partial sums in `workspace` (lr_alpha_hole_workspace_bytes),
 *                           reduced in a fixed order in double: bit-repeatable.
 *   lr_alpha_hole_backward: dL_dalpha [H,W] = upstream * weight * (1 - mask) / (H*W); `upstream` a device scalar or NULL for 1.
 *                           One elementwise pass, no workspace; it does not depend on alpha.
 * Deterministic (no atomics), no host synchronisation.  Return 0 or a negative LR_ERR_*.
 */
int lr_masked_l1_dssim_forward(int channels, int height, int width, const float* image, const float* gt, const float* mask,
                               float lambda_dssim, float* out_loss3, void* workspace, size_t workspace_bytes, void* stream);
int lr_masked_l1_dssim_backward(int channels, int height, int width, const float* image, const float* gt, const float* mask,
                                float lambda_dssim, const float* upstream, const void* workspace, float* dL_dimage, void* stream);
size_t lr_alpha_hole_workspace_bytes(int height, int width);
int lr_alpha_hole_forward(int height, int width, const float* alpha, const float* mask, float weight, float* out_loss,
                          void* workspace, size_t workspace_bytes, void* stream);
int lr_alpha_hole_backward(int height, int width, const float* mask, float weight, const float* upstream, float* dL_dalpha,
                           void* stream);

/*
 * Surface normals from a depth map, and the normal losses on them (luciddreamer_amd/csrc/normals.hip).
 *
 * depth: [H,W] float32 device image, contiguous: the rasterizer's depth or median depth, 0 = "no surface".  The camera is
 * tan_fovx, tan_fovy with the pixel convention of gauss_project.h: pixel (x, y) has the view-space ray (u, v, 1), axes x right,
 * y down, z forward.  Every operation below is ONE float32 operation in the order written (no fma; division and square root
 * correctly rounded), so a numpy float32 restatement gives the same bits (tests/normal_ref.py):
 *     ax = (2 tan_fovx) / W,  ay = (2 tan_fovy) / H
 *     u = ax (x + 0.5) - tan_fovx,  v = ay (y + 0.5) - tan_fovy
 * For an interior pixel (1 <= x <= W-2, 1 <= y <= H-2) with E, W, N, S the depths at (x+1,y), (x-1,y), (x,y-1), (x,y+1):
 *     gx = E - W,  sx = E + W,  gy = S - N,  sy = S + N
 *     p = ax sx,  r = ay sy
 *     a = r gx,  b = p gy
 *     c = ( a,  b,  -((b v + a u) + p r) )
 *     m2 = (c0 c0 + c1 c1) + c2 c2,  len = sqrt(m2),  n = ( c0 / len, c1 / len, c2 / len )
 * This is 2DGS's depth_to_normal: the normalised cross product of the central differences of the lifted points
 * P(x, y) = d(x, y) (u, v, 1), n ~ (P_S - P_N) x (P_E - P_W), oriented towards the camera (n.(u, v, 1) < 0).  It is NOT evaluated
 * by lifting and subtracting points: expanded, the cross product's terms in u^2, v^2 and u v cancel identically, and what is
 * left is written so that the only cancellation is the depth difference itself (gx, gy): the lifted form loses digits with the
 * resolution (neighbouring rays differ by ax), this one does not.  Because c.(u, v, 1) = -ax ay sx sy < 0, |c| > 0 whenever the
 * four depths are positive.  n(k depth) = n(depth) bit for bit for k a power of two.
 * A pixel is VALID when it is interior, its own depth and its four neighbours' depths are all > 0 (NaN fails), and m2 is finite
 * (and, against underflow, > 0).  An invalid pixel has the normal (0,0,0) and contributes nothing to any value or gradient.
 * H < 3 or W < 3 has no valid pixel: every output is exactly 0.
 *
 *   lr_depth_normals          : out_normals [3,H,W] = n (planes n0, n1, n2).
 *   lr_depth_normals_backward : dL_ddepth [H,W] from Gn = dL_dnormals [3,H,W]; per valid pixel
 *                                   dn = (n0 Gn0 + n1 Gn1) + n2 Gn2,   G_i = (Gn_i - n_i dn) / len
 *                               then the chain below.
 *   lr_normal_loss_forward    : loss = weight * sum_counted w_p (1 - n_p.t_p) / (H*W)  (divided by ALL pixels, as lr_depth_l1_forward),
 *                               out (device, 2 floats) = {loss, number of pixels that counted (exact up to 2^24)}.
 *                               pixel_weight: optional [H,W] plane w_p >= 0, NULL = 1; a value that is not > 0 (NaN included)
 *                               excludes the pixel.  The target is EXACTLY ONE of
 *                                   target_normals [3,H,W]: data, normalised here: tt = (t0 t0 + t1 t1) + t2 t2, tl = sqrt(tt),
 *                                       t = (t0 / tl, t1 / tl, t2 / tl); a pixel whose tt is not > 0 or not finite is excluded;
 *                                   target_depth [H,W]: t = its normals by the formula and validity rule above (the consistency
 *                                       term, e.g. expected depth against median depth).
 *                               A pixel COUNTS when its normal is valid, its target is, and its weight is.  Per pixel, float32:
 *                                   dot = (n0 t0 + n1 t1) + n2 t2,   term = w_p (1 - dot)
 *                               The terms are summed in double: per workgroup in a fixed order into `workspace`
 *                               (lr_normals_workspace_bytes), then by one workgroup in a fixed order.  No atomics: bit-repeatable.
 *   lr_normal_loss_backward   : dL_ddepth [H,W] = upstream * d loss / d depth; in consistency mode, optionally,
 *                               dL_dtarget_depth [H,W] = upstream * d loss / d target_depth: the same formula with the roles of
 *                               the two depths swapped.  `upstream` is a device scalar or NULL for 1.  The normals are recomputed
 *                               from the depths: no stored normal plane, no workspace.  Per counted pixel
 *                                   k = (upstream weight) / (float)(H W),   q = k w_p  (k without a weight plane)
 *                                   kk = q / len,   G_i = -(kk (t_i - n_i dot))
 * The chain from G to the four neighbour depths of a pixel:
 *     A = G0 - u G2,  B = G1 - v G2
 *     dgx = r A,  dgy = p B
 *     dsx = ax (gy B - r G2),  dsy = ay (gx A - p G2)
 *     tE = dgx + dsx,  tW = dsx - dgx,  tS = dgy + dsy,  tN = dsy - dgy
 * and the gradient is GATHERED, not scattered: output pixel (x, y) is
 *     ((tE of (x-1,y) + tW of (x+1,y)) + tS of (x,y-1)) + tN of (x,y+1)
 * -- the terms of its W, E, N and S neighbours' normals in that fixed order, a term of a pixel that does not count (or lies
 * outside the image) being +0.  No atomics: bit-repeatable.  A pixel's own normal does not depend on its own depth (only its
 * validity does), and the four image corners get exactly 0.
 *
 * height, width >= 1 and H*W < 2^31; tan_fovx, tan_fovy finite and > 0; weight finite and >= 0.  struct_bytes is checked before
 * anything else; every check sits in front of the first HIP call.  Each entry point reads the members named with it and ignores
 * the others.  No host synchronisation.  Return 0 or a negative LR_ERR_*.
 */
typedef struct lr_normals_args {
    size_t struct_bytes;                     /* = sizeof(lr_normals_args); anything else is LR_ERR_INVALID_ARG */
    int height, width;
    float tan_fovx, tan_fovy;
    const float* depth;                      /* all four: [H,W] */
    float* out_normals;                      /* lr_depth_normals: [3,H,W] */
    const float* dL_dnormals;                /* lr_depth_normals_backward: [3,H,W] */
    const float* target_normals;             /* loss forward / backward: [3,H,W], or */
    const float* target_depth;               /* ... [H,W]: exactly one of the two */
    const float* pixel_weight;               /* loss forward / backward: [H,W], optional */
    float weight;                            /* loss forward / backward */
    const float* upstream;                   /* loss backward: device scalar, optional */
    float* out;                              /* loss forward: {loss, count} */
    float* dL_ddepth;                        /* both backwards: [H,W] */
    float* dL_dtarget_depth;                 /* loss backward with target_depth: [H,W], optional */
    void* workspace;                         /* loss forward */
    size_t workspace_bytes;
    void* stream;
} lr_normals_args;
size_t lr_normals_workspace_bytes(int height, int width);
int lr_depth_normals(const lr_normals_args* a);
int lr_depth_normals_backward(const lr_normals_args* a);
int lr_normal_loss_forward(const lr_normals_args* a);
int lr_normal_loss_backward(const lr_normals_args* a);

/*
 * Edge-aware smoothness of a rendered map (luciddreamer_amd/csrc/smooth.hip): the first- or second-order smoothness term of
 * the Monodepth lineage / DNGaussian / MonoGS on a depth map, an inverse depth map or a normal map, gated by the edges of a
 * guide image.
 *
 * map: [C,H,W] float32 device image, contiguous, 1 <= C <= 4 (a depth map is C = 1, a normal map C = 3).  guide: optional
 * [G,H,W] image I, G = guide_channels in {1, 3} (guide_channels = 0 without one).  mask: optional [H,W] plane.
 * order in {1, 2}; space LR_SMOOTH_DIRECT or LR_SMOOTH_INVERSE; positive_only in {0, 1}; gamma, weight finite and >= 0.
 *
 * A pixel is VALID when every channel of `map` is finite, with positive_only its channel 0 is > 0 (the project's 0 = "no
 * surface"; NaN fails), and with a mask its mask value is > 0 (NaN fails).  The mask is a selector only: it is never multiplied
 * in.  The value used is u = map, in INVERSE space u = 1.0f / map (one float32 division); INVERSE needs C = 1 and positive_only
 * (anything else is LR_ERR_INVALID_ARG), and a pixel whose reciprocal is not finite (a subnormal depth) is invalid there.
 *
 * Order 1 has one term per horizontal pair (p, q = p + x) and one per vertical pair (p, q = p + y):
 *     a_g = |I_p,g - I_q,g|                                          float32, per guide channel
 *     a = a_0  (G = 1),   a = ((a_0 + a_1) + a_2) / 3.0f  (G = 3)
 *     w = expf(-(gamma a)),   w = 1 without a guide
 *     D_c = (double)u_q,c - (double)u_p,c
 *     term = (double)w * sum_c |D_c|                                  channels in order, double
 * Order 2 has one term per horizontal triple (m = p - x, p, q = p + x) and one per vertical triple:
 *     a_g = max(|I_p,g - I_m,g|, |I_q,g - I_p,g|)                    an edge on either side gates the term; a NaN on either side stays
 *     a, w as above
 *     D_c = ((double)u_m,c - 2.0 (double)u_p,c) + (double)u_q,c
 *     term = (double)w * sum_c |D_c|
 * A term COUNTS when all of its pixels are valid and a is finite: !(a >= 0) excludes a NaN, and a = +inf (an infinite guide
 * value on one side of the term) is excluded with it -- at gamma = 0 its weight would be expf(-(0 inf)) = NaN.
 *
 *   lr_smooth_forward  : loss = weight * (float)(S / (double)(H*W)), S the sum of the counted terms: divided by ALL pixels, as
 *                        lr_normal_loss_forward, never by a data-dependent number.  out (device, 2 floats) = {loss, number of
 *                        counted terms (exact up to 2^24)}.  Without a counted term (H = W = 1; order 2 with H, W < 3) both
 *                        are exactly 0.  The terms are summed in double: per lane (rows top to bottom, the horizontal term of a
 *                        pixel before its vertical one), per workgroup in a fixed order into `workspace`
 *                        (lr_smooth_workspace_bytes), then by one workgroup in a fixed order.  No atomics: bit-repeatable.
 *   lr_smooth_backward : dL_dmap [C,H,W] = upstream * d loss / d map; `upstream` is a device scalar or NULL for 1.  A GATHER:
 *                        a pixel adds the terms it belongs to, at most 4 at order 1 and 6 at order 2, their weights and signs
 *                        recomputed from the inputs (no stored plane, no workspace).  With
 *                            k = (upstream weight) / (float)(H W)
 *                        channel c of pixel p is g_u = k s, s the float32 sum of (coef w_t) sign(D_t,c) over its terms:
 *                        sign(0) = 0; coef = -1 for p and +1 for q at order 1, (1, -2, 1) for (m, p, q) at order 2, so both
 *                        products are exact.  The terms are added from +0 in this order: the horizontal ones from left to
 *                        right (order 1: the pair ending at the pixel, the pair starting at it; order 2: the triples centred
 *                        on x - 1, x, x + 1), then the vertical ones from top to bottom; a term that does not count adds
 *                        nothing.  k multiplies the SUM, once: multiples of k are not float32 numbers, small integers are,
 *                        so a pixel whose terms cancel as integers (w = 1 away from the guide's edges) gets an exact zero and
 *                        not the rounding residue of 3 k - 2 k - k.  INVERSE space then applies g_map = -(g_u u) u.  An invalid pixel, and a pixel without a counted term,
 *                        gets exactly 0.  The guide and the mask receive no gradient.  No atomics: bit-repeatable.
 *
 * Why the differences are formed in double: the gradient of an L1 term is nothing but the sign of its difference, and a float32
 * second difference can round to the wrong sign near zero.  The double operations are exact -- so the sign, and sign(0) = 0,
 * are those of the real-number difference -- whenever the magnitudes of the non-zero values of a term lie within a factor 2^27
 * of each other (values of 24 bits whose exponents differ by at most 27 leave m - 2p within the 53 bits of a double); beyond
 * that range the final addition is still correctly rounded, so a sign can be lost only where m - 2p itself was rounded.
 *
 * height, width >= 1 and H*W < 2^31.  struct_bytes is checked before anything else; every check (NULL pointers, sizes, channels,
 * guide_channels, order, space, positive_only, gamma, weight, workspace_bytes) sits in front of the first HIP call.  Each entry
 * point reads the members named with it and ignores the others.  No host synchronisation.  Return 0 or a negative LR_ERR_*.
 */
#define LR_SMOOTH_DIRECT  0
#define LR_SMOOTH_INVERSE 1
typedef struct lr_smooth_args {
    size_t struct_bytes;                     /* = sizeof(lr_smooth_args); anything else is LR_ERR_INVALID_ARG */
    int height, width;
    int channels;                            /* C of map and dL_dmap: 1..4 */
    int guide_channels;                      /* G of guide: 1 or 3; 0 without a guide */
    const float* map;                        /* [C,H,W] */
    const float* guide;                      /* [G,H,W], optional */
    const float* mask;                       /* [H,W], optional */
    int order;                               /* 1 or 2 */
    int space;                               /* LR_SMOOTH_DIRECT or LR_SMOOTH_INVERSE */
    int positive_only;                       /* 0 or 1 */
    float gamma;
    float weight;
    const float* upstream;                   /* backward: device scalar, optional */
    float* out;                              /* forward: {loss, count} */
    float* dL_dmap;                          /* backward: [C,H,W] */
    void* workspace;                         /* forward */
    size_t workspace_bytes;
    void* stream;
} lr_smooth_args;
size_t lr_smooth_workspace_bytes(int height, int width);
int lr_smooth_forward(const lr_smooth_args* a);
int lr_smooth_backward(const lr_smooth_args* a);

/*
 * Video frames on the device (the per-frame post-processing of the video renderer, R/luciddreamer.py:250-265).  Every entry
 * point takes n_frames contiguous frames of one H, W and handles them in the same launches; nothing reads back to the host.
 *
 *   lr_frames_to_u8 : images [n,3,H,W] float32 -> out [n,H,W,3] uint8,
 *                     out = uint8(rint(min(max(x, 0), 1) * 255))   (float32, round half to even, no fma; NaN -> 0)
 *                     = np.round(image.permute(1,2,0).numpy().clip(0,1) * 255.).astype(np.uint8) byte for byte.
 *   lr_depth_colorize : depths [n,H,W] float32 -> out_rgba [n,H,W,4] uint8, R/utils/depth.py:colorize with its defaults:
 *       v = from_render ? -(d * (d > 0)) : d;  valid = (v != invalid_val);  n = number of valid pixels
 *       vmin, vmax = np.percentile(v[valid], q_lo), np.percentile(v[valid], q_hi) in float32, "linear" method, bit for bit
 *                    (a NaN among the valid values gives NaN), found by a 3-pass radix select on the device (no sort);
 *                    or read from fixed_vmin_vmax (device float[2 * n]: vmin, vmax per frame; NULL = select) -- colorize(vmin=,
 *                    vmax=) with both limits given, taken as float32
 *       t = vmin != vmax ? (v - vmin) / (vmax - vmin) : v * 0;  x = t * lut_n, x == lut_n -> lut_n - 1
 *       colour = lut[trunc(x)], or row lut_n (under) for x < 0, lut_n + 1 (over) for x >= lut_n, lut_n + 2 (bad) for NaN;
 *       invalid pixels get background[0..3].
 *     lut: device uint8 [(lut_n + 3), 4], a matplotlib colormap's _lut with bytes=True (1 <= lut_n <= LR_VIDEO_MAX_LUT_N).
 *     background: HOST pointer to 4 bytes (RGBA).  out_vmin_vmax: device float[2 * n] (required): the limits used per frame.
 *     With n == 0 valid pixels (the reference raises IndexError) the frame is all background and vmin = vmax = NaN.
 *     workspace: lr_video_workspace_bytes(n_frames, H, W) device bytes (unused, and may be NULL, with fixed_vmin_vmax).
 *     The histograms merge with integer atomics only: the output is deterministic.
 * Images of at most 2^31 - 2^12 pixels, 1 <= n_frames <= 65535.  Return 0 or a negative LR_ERR_*.
 */
#define LR_VIDEO_MAX_LUT_N 4096
size_t lr_video_workspace_bytes(int n_frames, int height, int width);
int lr_frames_to_u8(int n_frames, int height, int width, const float* images, unsigned char* out, void* stream);
int lr_depth_colorize(int n_frames, int height, int width, const float* depths, int from_render, float invalid_val,
                      float q_lo, float q_hi, const float* fixed_vmin_vmax, const unsigned char* lut, int lut_n,
                      const unsigned char* background, unsigned char* out_rgba, float* out_vmin_vmax, void* workspace,
                      size_t workspace_bytes, void* stream);

/*
 * Point-cloud reprojection on the device (generate_pcd, R/luciddreamer.py:382-413 "Dreaming" and :516-570 "Aligning"): the
 * accumulated cloud projected into n_frames poses, every frame in the same launches; the warped image, the hit / hole masks of
 * the reference bit for bit, and the lift of a depth map back into the world.  Nothing reads back to the host.
 *
 *   Project.  x, y, z = the point's float32 coordinates as float64.  Every operation below is one IEEE float64 operation in the
 *   order written (no fma), so a numpy restatement gives the same bits (tests/reproject_ref.py):
 *       p_i = ((R_i0 x + R_i1 y) + R_i2 z) + T_i        q_i = (K_i0 p_0 + K_i1 p_1) + K_i2 p_2        u = q_0 / q_2, v = q_1 / q_2
 *       valid = q_2 > 0 and 0 <= u <= W - 1 and 0 <= v <= H - 1   (closed bounds; NaN is invalid)
 *       iu, iv = rint(u), rint(v)  (half to even, as np.round)    z = float32(q_2)
 *   Masks (the reference's, exactly).  hit[iv, iu] = 1;  dilated = 9x9 maximum of hit (round_mask2 / maskj after the filter);
 *   mask = 11x11 minimum of dilated (mask2 / maskj: the reference's (image.sum(-1) != -3) equals `dilated` whatever the image
 *   holds);  border = mask_hf of :411-413.  Windows are clamped to the image, which for maximum and minimum filters equals
 *   scipy's default `reflect` border.  out_valid[i] = valid, out_pix[i] = iv W + iu or -1: the caller's valid_idx,
 *   round_coord_cam2 and border_valid_idx follow from them by indexing.
 *   Image (OUR definition, not scipy.interpolate.griddata's Delaunay interpolation; the reference's has no occlusion handling):
 *   a z-tested bilinear splat in fixed point.
 *       zmin[y, x] = min z over the points that rounded to (x, y)  (atomicMin on the bits; +inf where there is none)
 *       x0, y0 = floor(u), floor(v);  fx, fy = u - x0, v - y0;  the neighbour (x0 + dx, y0 + dy), if inside the image, has
 *       w = (dx ? fx : 1 - fx) * (dy ? fy : 1 - fy) in float64,  wq = rint(w * 65536),
 *       cq_c = rint(float64(min(max(C_c, 0), 1)) * 65535)  (NaN -> 0),
 *       and is accepted iff z <= zmin[y', x'] * (1.0f + z_tolerance), float32 operations.
 *       A_c[y', x'] += wq cq_c and S[y', x'] += wq in uint64 (integer atomics: the sums do not depend on the order).
 *       A pixel with S == 0 takes the integer sums of A_c and S over its clamped 9x9 window (non-zero inside `dilated`: a hit
 *       pixel always has S >= 16384).
 *       image = float32((float64(A_c) / float64(S)) / 65535) inside mask, exact 0 outside (:409, :565), HWC;
 *       image_u8 = uint8(rint(image * 255.0f)) (:568);  depth = zmin inside mask where finite, else 0.
 *   The reference's `edgemask` patch (:400, :554) repairs griddata's hull edge and has no counterpart here.
 *
 *   points: device float32, the x of point i at points[i * point_stride], y and z coord_stride floats further each
 *   ([N,3]: 3, 1;  [3,N]: 1, N).  colors: device float32 [N,3], required when out_image or out_image_u8 is given.
 *   K [9], R [n_frames][9] (row-major), T [n_frames][3]: HOST float64, world to camera; all finite.
 *   Outputs are optional device pointers, frames contiguous: out_image float32 [F,H,W,3], out_image_u8 uint8 [F,H,W,3],
 *   out_mask / out_dilated / out_border uint8 [F,H,W], out_depth float32 [F,H,W]; out_valid uint8 [N] and out_pix int32 [N]
 *   only with n_frames == 1.  workspace: lr_reproject_workspace_bytes(n_frames, H, W) device bytes, 8-byte aligned.
 *   0 <= n_points < 2^31, 1 <= n_frames <= 65535, H, W >= 2 and H W <= 2^31 - 2^12; z_tolerance finite and >= 0.
 *   struct_bytes is checked before anything else; every check sits in front of the first HIP call.
 *
 *   lr_lift (:370-371, :451-453): depth [H,W] float32 -> out_points [3, H W] float32,
 *       c_i = (Kinv_i0 (x d) + Kinv_i1 (y d)) + Kinv_i2 d,   out_i = float32(((Rinv_i0 c_0 + Rinv_i1 c_1) + Rinv_i2 c_2) - RinvT_i)
 *   with x, y the pixel's column and row, x d and y d float64 products.  Kinv [9], Rinv [9], RinvT [3] (= inv(R) T): HOST
 *   float64, formed by the caller.
 * Return 0 or a negative LR_ERR_*.
 */
typedef struct lr_reproject_args {
    size_t struct_bytes;                     /* = sizeof(lr_reproject_args); anything else is LR_ERR_INVALID_ARG */
    long long n_points;
    const float* points;
    long long point_stride, coord_stride;    /* in floats */
    const float* colors;
    int n_frames, height, width;
    float z_tolerance;
    const double* K;                         /* host */
    const double* R;                         /* host */
    const double* T;                         /* host */
    float* out_image;
    unsigned char* out_image_u8;
    unsigned char* out_mask;
    unsigned char* out_dilated;
    unsigned char* out_border;
    float* out_depth;
    unsigned char* out_valid;
    int* out_pix;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} lr_reproject_args;
size_t lr_reproject_workspace_bytes(int n_frames, int height, int width);
int lr_reproject(const lr_reproject_args* a);
int lr_lift(int height, int width, const float* depth, const double* Kinv, const double* Rinv, const double* RinvT,
            float* out_points, void* stream);

/*
 * Dreaming on the device (generate_pcd, R/luciddreamer.py:424-493): once the networks have produced the new view's depth map D,
 * its scale against the cloud, the depth offsets along the hole's border, their interpolation into every hole pixel, and the
 * lift of the corrected depth.  The inputs are lr_reproject's of the same pose: out_valid, out_pix, and an index list formed from
 * out_border.  Nothing reads back to the host.
 *
 * All arithmetic is float64, one IEEE operation each in the order written (no fma), so a numpy restatement gives the same bits
 * (tests/dream_ref.py).  x, y are a pixel's column and row; Kinv, Rinv, RinvT as for lr_lift, K, R, T as for lr_reproject (one
 * pose), all HOST float64 and finite.
 *     liftw(x, y, d)_i = ((Rinv_i0 c_0 + Rinv_i1 c_1) + Rinv_i2 c_2) - RinvT_i,   c_i = (Kinv_i0 (x d) + Kinv_i1 (y d)) + Kinv_i2 d
 *   (lr_lift's formula without its rounding to float32).  a.b = (a_0 b_0 + a_1 b_1) + a_2 b_2.
 *
 *   lr_dream_scale_sums (:424-440; what the reference meant to fit: its 100 Adam steps act on a leaf that is rebuilt from the
 *   scale's VALUE every step, so the scale never receives a gradient and stays 1).  For every point i with valid[i] != 0 and
 *   0 <= pix[i] < H W:  P = the point as float64,  q = liftw(pix_i % W, pix_i / W, D[pix_i]);  a pair whose q has a non-finite
 *   component is left out.  out_sums = {sum P.P, sum P.q, sum q.q} (device, 3 doubles), out_count = the number of pairs (device,
 *   one long long).  The minimiser of mean |P - s q|^2 is s = Spq / Sqq.  Summation order: thread t of workgroup b holds the
 *   term of point 256 b + t (0 where there is none); for st = 128, 64, ..., 1: term[t] += term[t + st] for t < st; then the
 *   workgroup sums are added in index order.  No float atomics: two runs give the same bits.
 *   workspace: lr_dream_workspace_bytes(n_points) device bytes, 8-byte aligned.
 *
 *   lr_dream_correspond (:443-474).  corr [n_corr] int32 (device, ascending): indices of cloud points on the hole's border.  For
 *   j < n_corr, i = corr[j]:  u, v = lr_reproject's exact projected coordinates of point i (the same operations),
 *       c = scale * liftw(pix_i % W, pix_i / W, D[pix_i])  (componentwise),   o = -RinvT,  a = c - o,  p = P_i - o,
 *       t = (p.a) / (a.a),   m = o + a t,   value_j = rowz(m) - rowz(c),   rowz(X) = ((R_20 X_0 + R_21 X_1) + R_22 X_2) + T_2:
 *   how far along the camera ray the new depth is from the foot of the cloud point.  a.a == 0, a non-finite value_j or a pix_i
 *   outside [0, H W) gives value_j = NaN (the sample is skipped downstream); an i outside [0, n_points) gives NaN in all three.
 *   out_su, out_sv, out_sval: device double [n_corr + 4]; the last four are the corners (0,0), (0,H-1), (W-1,0), (W-1,H-1) with
 *   value 0, in that order (:469-474).
 *
 *   lr_scatter_interpolate (OUR definition, in place of :478-479's scipy.interpolate.griddata: linear over a Delaunay
 *   triangulation with a nearest-neighbour fallback).  A moving least squares fit of an affine function with inverse-distance
 *   weights.  n_samples >= 0 samples (su, sv, sval), device double; a pixel is a query iff its byte of where [H,W] is 0.  For a
 *   query (x, y), over the samples in index order, skipping those whose sval is NaN:
 *       dx = su_j - x,  dy = sv_j - y,  d2 = (dx dx + dy dy) + 1e-12,  w = 1.0 / (d2 d2),  wx = w dx,  wy = w dy,  wv = w sval_j
 *       S00 += w, S01 += wx, S02 += wy, S11 += wx dx, S12 += wx dy, S22 += wy dy;   B0 += wv, B1 += wv dx, B2 += wv dy
 *       vmin, vmax = the smallest and largest sval_j
 *   then  C0 = S11 S22 - S12 S12,  C1 = S02 S12 - S01 S22,  C2 = S01 S12 - S02 S11,
 *       det = (S00 C0 + S01 C1) + S02 C2,   num = (B0 C0 + B1 C1) + B2 C2,
 *       r = num / det  if det > 1e-12 ((S00 S11) S22),  else B0 / S00  (Shepard's weighted mean: collinear samples, a query on a
 *       sample),   t = r > vmin ? r : vmin,   t = t < vmax ? t : vmax   (the affine fit overshoots outside the samples' hull; a
 *       NaN r takes vmin),   out = float32(t).
 *   out is 0 where where != 0 or where no sample was usable.  The accumulation is sequential in j: bit-repeatable.  Samples are
 *   staged on chip in tiles of LR_SCATTER_TILE.
 *
 *   lr_dream_lift (:481-489).  dd = float64(D[y,x]) + float64(new_depth[y,x]),  out_i = float32(scale * liftw(x, y, dd)_i),
 *   out_points [3, H W].  The reference lifts D and new_depth separately, adds, rounds to float32 and then scales; this rounds
 *   once.  With new_depth = 0 and scale = 1 the result is lr_lift's, bit for bit.
 *
 *   0 <= n_points < 2^31, 0 <= n_corr <= 2^31 - 5, 0 <= n_samples < 2^31, H, W >= 1 and H W <= 2^31 - 2^12; scale finite.
 *   struct_bytes is checked before anything else; every check sits in front of the first HIP call.  Each entry point reads the
 *   members named with it and ignores the others.  Return 0 or a negative LR_ERR_*.
 */
#define LR_SCATTER_TILE 256
typedef struct lr_dream_args {
    size_t struct_bytes;                     /* = sizeof(lr_dream_args); anything else is LR_ERR_INVALID_ARG */
    long long n_points;                      /* scale_sums, correspond */
    const float* points;                     /* scale_sums, correspond: as lr_reproject_args */
    long long point_stride, coord_stride;
    const unsigned char* valid;              /* scale_sums: lr_reproject's out_valid [N] */
    const int* pix;                          /* scale_sums, correspond: lr_reproject's out_pix [N] */
    int height, width;
    const float* depth;                      /* all three: D [H,W] */
    const double* K;                         /* correspond; host */
    const double* R;                         /* correspond; host */
    const double* T;                         /* correspond; host */
    const double* Kinv;                      /* all three; host */
    const double* Rinv;                      /* all three; host */
    const double* RinvT;                     /* all three; host */
    double scale;                            /* correspond, lift */
    const int* corr;                         /* correspond: [n_corr] */
    long long n_corr;
    double* out_su;                          /* correspond: [n_corr + 4] each */
    double* out_sv;
    double* out_sval;
    double* out_sums;                        /* scale_sums: [3] */
    long long* out_count;                    /* scale_sums: [1] */
    const float* new_depth;                  /* lift: [H,W] */
    float* out_points;                       /* lift: [3, H W] */
    void* workspace;                         /* scale_sums */
    size_t workspace_bytes;
    void* stream;
} lr_dream_args;
typedef struct lr_scatter_args {
    size_t struct_bytes;                     /* = sizeof(lr_scatter_args); anything else is LR_ERR_INVALID_ARG */
    long long n_samples;
    const double* su;                        /* [n_samples] each; may be NULL when n_samples == 0 */
    const double* sv;
    const double* sval;
    int height, width;
    const unsigned char* where;              /* [H,W]: 0 = query */
    float* out;                              /* [H,W] */
    void* stream;
} lr_scatter_args;
size_t lr_dream_workspace_bytes(long long n_points);
int lr_dream_scale_sums(const lr_dream_args* a);
int lr_dream_correspond(const lr_dream_args* a);
int lr_dream_lift(const lr_dream_args* a);
int lr_scatter_interpolate(const lr_scatter_args* a);

/*
 * TSDF fusion of depth maps and mesh extraction on the device (csrc/tsdf.hip): what the surface-reconstruction code bases do
 * with Open3D on the host after rendering depth along a trajectory.  The definitions are OURS; every float32 operation below is
 * one IEEE operation in the order written (no fma), so a numpy restatement gives the same bits (tests/tsdf_ref.py).
 *
 *   Volume.  origin (3 floats), voxel_size s > 0, dims nx, ny, nz >= 2, trunc > 0.  Samples sit at the lattice points
 *   c = origin + s (i, j, k), each coordinate float32(i) * s + origin (one multiply, then one add).  Three device tensors, x
 *   fastest: tsdf [nz,ny,nx] float32 (initially 1), weight [nz,ny,nx] float32 (initially 0), color [nz,ny,nx,3] float32
 *   (initially 0); the linear index of a lattice point is (k ny + j) nx + i.  7 nx ny nz <= 2^31 - 2^12 (an edge id is an int;
 *   the scan reads whole tiles).
 *
 *   Integrate (lr_tsdf_integrate).  n_frames frames: depth [F,H,W] float32, optional color [F,H,W,3] and pixel_weight [F,H,W]
 *   float32; K [9], R [F][9], T [F][3] HOST float64, world to camera, as for lr_reproject.  For every lattice point the frames
 *   are applied in index order; for each frame
 *       project the float32 point as lr_reproject does (float64, the same operations, valid test and rint); skip if not valid;
 *       d = depth[f, iv, iu]; skip unless d is finite, d > 0 and d <= depth_max;
 *       w = pixel_weight[f, iv, iu], or 1 without the map; skip unless w is finite and w > 0;
 *       sdf = d - z with z = float32(q_2); skip if sdf < -trunc;   v = min(1, sdf / trunc);   Wn = W + w;
 *       D = (D W + v w) / Wn, and each colour channel C = (C W + c w) / Wn;   W = min(Wn, max_weight).
 *   Without a colour stack the colour tensor is not touched; a voxel no frame reached is not written.  A gather, one writer per
 *   voxel, no atomics: bit-repeatable, and n frames in one call equal the same frames in n calls bit for bit.
 *   H, W >= 2 and H W <= 2^31 - 2^12; 1 <= n_frames <= 65535; depth_max > 0 and max_weight > 0 (either may be +inf).
 *
 *   Extract (lr_tsdf_extract_count, then lr_tsdf_extract_emit).  A cell is the cube with minimum corner (i, j, k); it is valid
 *   when all eight corners have weight >= min_weight.  A lattice point is inside iff tsdf < 0 (a stored 0 is outside).  Each
 *   valid cell is split into the six Kuhn tetrahedra along the diagonal (0,0,0)-(1,1,1): for every permutation (a, b, c) of
 *   the axes in lexicographic order, v0 = 0, v1 = e_a, v2 = e_a + e_b, v3 = (1,1,1).  Per tetrahedron:
 *       one vertex l alone on its side, the others o0 < o1 < o2: the triangle (l o0, l o1, l o2);
 *       inside p < q, outside r < s: the quad pr, ps, qs, qr as (pr, ps, qs) and (pr, qs, qr).
 *   Winding is combinatorial: a triangle (x, y, z) is emitted as (x, z, y) when, with every vertex at its edge's midpoint, the
 *   normal of (x, y, z) would point from the outside vertices to the inside ones.  That follows from the permutation's parity
 *   and the inside mask alone; computed positions are never consulted (a stored 0 gives triangles of zero area).
 *   Vertices are welded: an edge is (lower lattice point, direction), the directions being (1,0,0) (0,1,0) (0,0,1) (1,1,0)
 *   (1,0,1) (0,1,1) (1,1,1), its id 7 (linear index of the lower point) + direction; the vertex list holds, in ascending id,
 *   exactly the edges some emitted triangle uses.  With p the lower point, t = D_p / (D_p - D_q), and each component of the
 *   position and of the colour is x_p + t (x_q - x_p) (subtract, multiply, add).  Faces are int32 [T,3], ordered by the linear
 *   index of the cell's minimum corner, then tetrahedron 0..5, then triangle.
 *   count fills the workspace, writes the two sizes to HOST memory and costs one stream synchronisation; the caller allocates
 *   out_vertices [V,3], out_colors [V,3] float32 and out_faces [T,3] int32 and passes the sizes back to emit with the SAME
 *   workspace and an unchanged volume.  A size of 0 needs no pointer.  LR_ERR_OVERFLOW when 3 T does not fit an int32.
 *   workspace: lr_tsdf_workspace_bytes(a) device bytes (dims read from a->vol; 0 for dims it refuses), 40 per lattice point.
 *
 *   Every device pointer must be 16-byte aligned.  struct_bytes is checked before anything else; every check sits in front of
 *   the first HIP call.  Return 0 or a negative LR_ERR_*.
 */
typedef struct lr_tsdf_volume {
    float origin[3];
    float voxel_size;
    int nx, ny, nz;
    float trunc;
    float* tsdf;
    float* weight;
    float* color;
} lr_tsdf_volume;
typedef struct lr_tsdf_integrate_args {
    size_t struct_bytes;                     /* = sizeof(lr_tsdf_integrate_args); anything else is LR_ERR_INVALID_ARG */
    lr_tsdf_volume vol;
    int n_frames, height, width;
    const float* depth;
    const float* color;                      /* optional */
    const float* pixel_weight;               /* optional */
    const double* K;                         /* host */
    const double* R;                         /* host */
    const double* T;                         /* host */
    float depth_max, max_weight;
    void* stream;
} lr_tsdf_integrate_args;
typedef struct lr_tsdf_extract_args {
    size_t struct_bytes;                     /* = sizeof(lr_tsdf_extract_args); anything else is LR_ERR_INVALID_ARG */
    lr_tsdf_volume vol;
    float min_weight;                        /* count; not NaN */
    void* workspace;
    size_t workspace_bytes;
    long long* out_n_vertices;               /* count: HOST */
    long long* out_n_faces;                  /* count: HOST */
    long long n_vertices, n_faces;           /* emit: what count returned */
    float* out_vertices;                     /* emit */
    float* out_colors;                       /* emit */
    int* out_faces;                          /* emit */
    void* stream;
} lr_tsdf_extract_args;
size_t lr_tsdf_workspace_bytes(const lr_tsdf_extract_args* a);
int lr_tsdf_integrate(const lr_tsdf_integrate_args* a);
int lr_tsdf_extract_count(const lr_tsdf_extract_args* a);
int lr_tsdf_extract_emit(const lr_tsdf_extract_args* a);

/*
 * Mesh clean-up on the device (csrc/mesh.hip): what the same code bases do with Open3D on the host after extraction --
 * cluster_connected_triangles, keep the largest clusters, remove_unreferenced_vertices, remove_degenerate_triangles,
 * compute_vertex_normals.  The definitions are OURS, stated so that a numpy restatement gives the same bits (tests/mesh_ref.py).
 *
 *   Inputs.  vertices [V,3] float32, faces [T,3] int32, optional per-vertex colors and normals [V,3] float32;
 *   0 <= V, T <= 2^31 - 2^12.  A face with an index outside [0, V) is OUT OF RANGE: no kernel dereferences it, it belongs to no
 *   component and is never kept.
 *
 *   Components (lr_mesh_components).  Two vertices are connected when an in-range face holds both (vertex connectivity; Open3D
 *   connects triangles across shared edges: the two differ only at a pinch vertex).  vertex_labels[v] is the smallest vertex
 *   index of v's component; an unreferenced vertex is its own label.  face_labels[t] = vertex_labels[faces[t,0]], or -1 for an
 *   out-of-range face.  component_faces[l] is the number of in-range faces with label l (0 where l is no label).  A canonical
 *   label and integer counts: no output depends on an arrival order.
 *
 *   Filter (lr_mesh_filter_count, then lr_mesh_filter_emit) with keep_largest K >= 0, min_faces M >= 1, drop_degenerate.
 *   Let c_1 >= c_2 >= ... be the face counts of the C components that have at least one face; kth = c_K if 1 <= K <= C, else
 *   0; threshold = max(kth, M).  A face is kept iff it is in range, component_faces[label] >= threshold, and, with
 *   drop_degenerate, it is not degenerate.  Ties at the threshold are all kept (2DGS's post_process_mesh rule, with a defined
 *   K > C case).  A face is degenerate when two of its indices are equal or when L below is 0 or not finite; the counts are
 *   taken before degenerate faces are dropped.  A vertex is kept iff a kept face refers to it.  Kept vertices and kept faces
 *   stay in input order, faces are re-indexed; out_vertex_index [V'] and out_face_index [T'] (optional) are the source rows.
 *   count fills the workspace, writes V' and T' to HOST memory and costs one stream synchronisation; the caller allocates the
 *   outputs and passes the sizes back to emit with the SAME workspace and unchanged inputs.  A size of 0 needs no pointer.
 *   out_colors / out_normals are required exactly when colors / normals are given.
 *
 *   Vertex normals (lr_mesh_vertex_normals): Open3D's compute_vertex_normals, equal weights over unit face normals.  Per
 *   in-range face, in float64, one IEEE operation per step, no fma: a, b, c the three vertices converted to double,
 *   e1 = b - a, e2 = c - a, n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), L = sqrt((nx nx + ny ny) + nz nz).
 *   If L is finite and > 0 the face adds q = (int64) rint(n / L * 2^20) to each of its three vertices, otherwise nothing.  The
 *   sums are int64 (integer addition is associative: no dependence on the face order).  Per vertex s = (double) sum,
 *   S = sqrt((sx sx + sy sy) + sz sz); the normal is (float)(s / S), or (0,0,0) when S == 0.
 *
 *   workspace: lr_mesh_workspace_bytes(V, T) device bytes for any of the calls (0 for sizes it refuses): 24 per vertex and 9
 *   per face, plus alignment.
 *
 *   Every device pointer must be 16-byte aligned.  struct_bytes is checked before anything else; every check sits in front of
 *   the first HIP call.  V = 0 and T = 0 are valid (nothing is launched over zero items; a size of 0 needs no pointer).
 *   Return 0 or a negative LR_ERR_*.
 */
typedef struct lr_mesh_components_args {
    size_t struct_bytes;                     /* = sizeof(lr_mesh_components_args); anything else is LR_ERR_INVALID_ARG */
    long long n_vertices, n_faces;
    const int* faces;
    int* vertex_labels;                      /* out [V] */
    int* face_labels;                        /* out [T] */
    int* component_faces;                    /* out [V] */
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} lr_mesh_components_args;
typedef struct lr_mesh_filter_args {
    size_t struct_bytes;                     /* = sizeof(lr_mesh_filter_args); anything else is LR_ERR_INVALID_ARG */
    long long n_vertices, n_faces;
    const float* vertices;
    const int* faces;
    const float* colors;                     /* optional */
    const float* normals;                    /* optional */
    int keep_largest, min_faces, drop_degenerate;
    void* workspace;
    size_t workspace_bytes;
    long long* out_n_vertices;               /* count: HOST */
    long long* out_n_faces;                  /* count: HOST */
    long long n_out_vertices, n_out_faces;   /* emit: what count returned */
    float* out_vertices;                     /* emit */
    float* out_colors;                       /* emit, with colors */
    float* out_normals;                      /* emit, with normals */
    int* out_faces;                          /* emit */
    int* out_vertex_index;                   /* emit, optional */
    int* out_face_index;                     /* emit, optional */
    void* stream;
} lr_mesh_filter_args;
typedef struct lr_mesh_normals_args {
    size_t struct_bytes;                     /* = sizeof(lr_mesh_normals_args); anything else is LR_ERR_INVALID_ARG */
    long long n_vertices, n_faces;
    const float* vertices;
    const int* faces;
    float* out_normals;                      /* out [V,3] */
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} lr_mesh_normals_args;
size_t lr_mesh_workspace_bytes(long long n_vertices, long long n_faces);
int lr_mesh_components(const lr_mesh_components_args* a);
int lr_mesh_filter_count(const lr_mesh_filter_args* a);
int lr_mesh_filter_emit(const lr_mesh_filter_args* a);
int lr_mesh_vertex_normals(const lr_mesh_normals_args* a);

/* present[P] (1 byte each) = view-space z > 0.2.  Returns 0 or a negative LR_ERR_*. */
int lr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                    unsigned char* present, void* stream);

/* Synchronises `stream` and reports the header state of a geom buffer written by lr_forward:
 * num_rendered via *num_rendered (may be NULL); returns 0, LR_ERR_OVERFLOW or LR_ERR_PREFILTERED. */
int lr_check(const char* geom_buffer, long long* num_rendered, void* stream);

/* The same without blocking (async mode's deferred overflow check): lr_header_post enqueues, on `stream`, a copy of the
 * first 8 header words {num_rendered, overflow, prefilter trap, capacity, P, num_sorted, num_instances, bin_bound} into
 * pinned memory owned by the library and returns a ticket >= 0 (or a negative LR_ERR_*).  lr_header_poll(ticket, block,
 * out8) returns 1 and fills out8 once the copy has completed (the ticket is then released), 0 if it has not and
 * block == 0, a negative LR_ERR_* on a bad ticket.  The device current at lr_header_post must be the buffer's. */
long long lr_header_post(const char* geom_buffer, void* stream);
/* "Verify in the forward": lr_request_early_header() makes the next async-mode lr_forward / lr_view_forward on the calling
 * thread post such a ticket itself as soon as the view's counts are final -- after the compaction scan, with the binning and
 * blend kernels enqueued behind it -- and lr_take_early_ticket() hands it out (-1: none, e.g. exact mode or P == 0).  A caller
 * that polls it with block = 1 right after lr_forward returns waits only for the preprocess and scan kernels (the host has
 * enqueued the rest of the forward meanwhile, so the GPU does not idle as it does during exact mode's read-back) and knows
 * before it hands the image to anyone whether the view overflowed; if so it calls lr_forward again with binning_capacity = 0.
 * The Python operator's default policy. */
void lr_request_early_header(void);
long long lr_take_early_ticket(void);
int lr_header_poll(long long ticket, int block, unsigned int* out8);

/* Ticket of the header of the LAST async-mode (binning_capacity > 0) lr_forward / lr_view_forward on the calling thread, for
 * lr_header_poll -- or -1 (no such forward yet, exact mode, P == 0).  Costs nothing: async-mode forwards leave their header in
 * a ring of host-visible slots written by the scan kernel itself (no copy, no event; the poll spins on the slot's tag), which
 * is what a caller that keeps several views in flight checks its views with (luciddreamer_amd/config.py).  The slot of a
 * ticket is re-used after 4096 further forwards on the device. */
long long lr_forward_ticket(void);
/* A STEP of several views issued through the per-view entry points (what lr_views_accumulate is for callers that need the
 * rendered image between forward and backward).  Between lr_step_begin and lr_step_end on a device, every accumulate-mode
 * lr_backward / lr_view_backward whose accumulate_mask covers mean2D, opacity, mean3D, scale and rotation (and that uses neither
 * colors_precomp nor cov3D_precomp) adds those five rows into ONE interleaved 64-byte row per Gaussian owned by the library
 * instead of five scattered 12-16 byte read-modify-writes; lr_step_end(stream) adds the touched rows into the five tensors
 * the step's calls named (calls that name other tensors, or another P, accumulate directly as before).  The calls of a step
 * must be ordered among themselves -- one stream, or lr_backward_wait_event chaining -- as accumulate-mode calls into shared
 * tensors must be anyway; `stream` of lr_step_end must be ordered after all of them.  Returns 0 or a negative LR_ERR_*. */
int lr_step_begin(void);
int lr_step_end(void* stream);
/* Close a step WITHOUT handing its rows over: for a step that was abandoned (error in the caller's loop, a begin whose end never
 * came).  The tensors named by its views may be gone by then; nothing is written through the remembered pointers. */
int lr_step_abort(void);
/* Accumulate-mode backward passes of different views on different streams add into the SAME gradient tensors and must not
 * overlap there.  `event` (a hipEvent_t, or NULL) is consumed by the next lr_backward / lr_view_backward on the calling thread:
 * its stream waits for the event after the blend backward (which writes only the call's own scratch) and before the kernels
 * that touch the outputs -- so a caller that records an event after each backward and passes it to the next one chains the
 * accumulations while the blend backward of one view still overlaps the per-Gaussian backward of the previous one
 * (csrc/torch_ext.cpp does this for the autograd operator; lr_views_accumulate does it internally). */
void lr_backward_wait_event(void* event);
/* Diagnostics: switch a kernel variant at run time (benchmark tooling measures two variants alternately in one process).
 * Knobs: "bwd_red" (reduction variant of the blend backward), "blend_quad", "tile_map", "preprocess", "gauss_bwd", "tsort",
 * "walk_own" (instances of a Gaussian the binning walks on its own lane), "hit_mask" (0: binning without preprocess's tile masks);
 * value -1 restores the library's own rule.  Results are identical up to float summation order whatever the setting.
 * Not part of the reference interface (it has no equivalent). */
/* Test hook: force one of the SHIPPED code paths that the library otherwise picks by rule (value -1 = the rule again).
 * Results never depend on it beyond float rounding between kernel shapes; the parity suite runs every path through it.
 *   "strict" 1           the blend in the reference's own float operations (luciddreamer_amd.config.set_strict_parity)
 *   "views_in_flight" n  hint: the caller keeps n views' kernels in flight on different streams (parallel.ViewStreams)
 *   "blend_quad" 0/1/2   blend backward: 2 waves per tile / 4 waves per tile / 1 wave per tile
 *   "fwd_pair" 0/2       blend forward: quadrant kernel / 1 wave per tile
 *   "tile_map" 0/1       tile -> workgroup map: XCD bands / plain
 *   "bwd_seg" 0          the blend backward walks whole lists instead of 256-position segments
 *   "bwd_red" 4          every wave of the blend backward takes the loop copy with the `pos < last` test
 *   "preprocess" 0/1     plain / pooled preprocess kernel;  "hit_mask" 0: no tile masks;  "walk_own" n: binning
 *   "tsort" 0..4         per-bin sort of the binning, bins of up to 256 entries (one wave): 0 bitonic network (also for 257..1024);
 *                        1 the same, bucket sort for 257..1024; 2 network up to 64 entries, bucket sort above; 3 rank sort for all of
 *                        them; 4 rank sort up to 128 entries, bucket sort above.  The rule (-1) is 4.  Every setting writes the same
 *                        lists.
 *   "bin_fuse" 0/1       per-bin sort of the binning in async mode: 0 two launches (bins up to 1024 entries, then the queue of the
 *                        larger ones), 1 one launch where the binning capacity says that the average bin holds at most 256 entries
 *                        (the small sort's workgroups then serve the queue too).  The rule (-1) is 1.  Exact mode always has two.
 *                        Every setting writes the same lists.
 *   "blend_fuse" 0/1/2   lr_views_accumulate, a view with a fixed dL_dpix as its only upstream gradient whose image, depth and alpha
 *                        nobody reads: 0 blend forward and backward as two launches; 1 one launch (the forward and the backward of
 *                        a tile in one wave) where both would be the one-wave-per-tile kernels; 2 one launch at every image size
 *                        and with any number of views in flight.  The rule (-1) is 1.  Every setting computes the same bits.
 *   "gauss_bwd" 0        no interleaved step accumulator
 * Values that select a RETIRED kernel ("part_scan", "bwd_red" 0 / 2 / 3, "fwd_pair" 1) and every LR_* environment override exist only in the
 * diagnostics build (-DLR_DIAGNOSTICS, `python -m luciddreamer_amd.build --diagnostics`; lr_version() then says "+diagnostics");
 * the product library rejects them with LR_ERR_INVALID_ARG and reads no environment variable. */
int lr_tune_set(const char* name, int value);
/* Anti-aliasing (the `antialiasing` switch of the upstream 3DGS rasterizer, the 2D Mip filter of Mip-Splatting).  Preprocess
 * dilates every screen-space covariance {a0, b, c0} by h = 0.3 on its diagonal; with the setting on it also multiplies the
 * opacity it stores for the blend by
 *     coef = sqrt(max(0.000025, det0 / det)),   det0 = a0 c0 - b b,   det = (a0 + h)(c0 + h) - b b,
 * so that a splat smaller than a pixel is dimmed by as much as the dilation spreads it.  Radii, tile rectangles, conics and
 * depths do not move; colour, depth, alpha and every gradient follow from the scaled opacity (the backward adds the
 * coefficient's derivative with respect to the covariance to dL/dmeans3D, dL/dscales, dL/drotations or dL/dcov3D).
 * A PROCESS-WIDE setting (not per thread: an autograd engine runs backwards on threads other than the forward's), 0 = off by
 * default, and then no output differs by a bit from a library without it.  Unlike lr_tune_set it changes results.  Every entry
 * point reads it once when it starts: lr_forward, lr_backward, lr_view_forward, lr_view_backward, and every view of the lr_views_* family.
 * CONTRACT: a view's backward must run under the setting its forward ran under -- the geom buffer holds the scaled opacity and
 * nothing records which kind it is; the gradients of a mixed pair are silently wrong.  (luciddreamer_amd's autograd functions
 * remember the forward's setting and raise instead.)  Do not toggle it while an lr_views_* call is running.
 * lr_set_antialiasing returns the previous value. */
int lr_set_antialiasing(int on);
int lr_get_antialiasing(void);
/* Kernel shapes of the process's last blend launches (either pointer may be NULL): forward 0 quadrant kernel, 1 with
 * candidate pairs, 2 one wave per tile; backward 0 two waves per tile, 1 four, 2 one; -1 = none yet.  For tests that must
 * know WHICH kernels a configuration ran (e.g. that the headline's step ran the one-wave-per-tile pair). */
int lr_last_launch_shapes(int* forward_shape, int* backward_shape);
/* Channel set of the process's last blend forward (the pointer may be NULL): LR_FWD_CHANNEL_COLOR | LR_FWD_CHANNEL_DEPTH for a
 * forward that blends colour and depth, LR_FWD_CHANNEL_COLOR for a depth-free one, 0 for the colour-free forward of
 * lr_views_accumulate (see lr_views_args::out_color); -1 = none yet.  For tests that must know that the colour-free kernel ran. */
#define LR_FWD_CHANNEL_COLOR 1
#define LR_FWD_CHANNEL_DEPTH 2
int lr_last_forward_channels(int* channels);
/* Optional per-stage timing with HIP events recorded on the call's stream (bench.py roofline leg).
 * lr_profile_enable(1) clears and starts recording, (0) stops; returns the number of stages.
 * lr_profile_read waits for the recorded events and returns, per stage, the summed elapsed
 * milliseconds and the number of recorded calls.  Stage names: lr_profile_stage_name(i).
 * The stages "preprocess", "render_fwd", "render_bwd", "gauss_bwd" are exactly one kernel launch each. */
int lr_profile_enable(int on);
const char* lr_profile_stage_name(int stage);
int lr_profile_read(double* ms_per_stage, long long* calls_per_stage, int n_stages);

/* Mean squared distance to the 3 nearest other points (simple-knn distCUDA2).
 * points [P,3] -> out [P].  workspace: lr_dist2_workspace_bytes(P) device bytes. */
size_t lr_dist2_workspace_bytes(int P);
int lr_dist2(int P, const float* points, float* out, char* workspace, void* stream);
/* For tests of the Morton stage: byte offsets inside `workspace` of what lr_dist2 leaves there once its work on the stream is
 * done -- offsets[0] the sorted 30-bit Morton keys (uint32 [P]), [1] the order (original index of every sorted position,
 * uint32 [P]), [2] the points in that order (float4 [P]: x, y, z, the original index's bits), [3] the boxes (float [ceil(P/256)][8]:
 * min xyz, unused, max xyz, unused; box b covers sorted positions 256 b .. 256 b + 255).  Pure host function; the layout is an
 * implementation detail and may change with the library version. */
int lr_dist2_workspace_layout(int P, size_t offsets[4]);

#ifdef __cplusplus
}
#endif
#endif /* LUCID_RASTER_H_INCLUDED */
