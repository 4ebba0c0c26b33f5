/*
 * gsr.h -- C ABI of the MI355X (gfx950) differentiable Gaussian tile rasterizer.
 *
 * This is the drop-in boundary for the reference's native rasterizer
 * (mango1118/gaussian_splatting, submodules/diff-gaussian-rasterization).  Each
 * entry point replaces one C++ interface of the reference:
 *
 *   gsr_rasterize_forward   <- CudaRasterizer::Rasterizer::forward
 *                              (cuda_rasterizer/rasterizer.h:31-58,
 *                               cuda_rasterizer/rasterizer_impl.cu:227-370)
 *   gsr_rasterize_backward  <- CudaRasterizer::Rasterizer::backward
 *                              (cuda_rasterizer/rasterizer.h:60-91,
 *                               cuda_rasterizer/rasterizer_impl.cu:374-479)
 *   gsr_mark_visible        <- CudaRasterizer::Rasterizer::markVisible
 *                              (cuda_rasterizer/rasterizer.h:23-29,
 *                               cuda_rasterizer/rasterizer_impl.cu:169-181)
 *
 * and, one layer up, the three pybind functions of ext.cpp:15-19
 * (rasterize_gaussians / rasterize_gaussians_backward / mark_visible), whose
 * tensor handling lives in the Python host layer (gaussian_splatting_amd/_C.py).
 *
 * Conventions (same as the reference):
 *  - every float array is a device pointer to contiguous fp32 data; an absent
 *    optional input is NULL (the reference's data_ptr() == nullptr test);
 *  - viewmatrix / projmatrix are 16 floats read column-major
 *    (cuda_rasterizer/auxiliary.h:75-95);
 *  - the three scratch buffers are obtained through allocation callbacks exactly
 *    like the reference's std::function<char*(size_t)> resize functors
 *    (rasterize_points.cu:29-43); their contents are private to this library and
 *    must be passed back unchanged to gsr_rasterize_backward;
 *  - all work is enqueued on `stream` (a hipStream_t; NULL = the default stream).
 *    gsr_rasterize_forward waits on it once, to learn the number of tile instances
 *    (cuda_rasterizer/rasterizer_impl.cu:313; see gsr_forward_args.capacity_hint).
 *
 * Every function returns 0 on success or a nonzero GSR_ERR_* code; the message
 * of the last failure on the calling thread is available from gsr_last_error().
 */
#ifndef GSR_H_INCLUDED
#define GSR_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_OK 0
#define GSR_ERR_ARGUMENT 1      /* invalid argument (shape, size, null pointer) */
#define GSR_ERR_HIP 2           /* a HIP runtime / kernel launch error */
#define GSR_ERR_ALLOC 3         /* an allocation callback returned NULL */
#define GSR_ERR_OVERFLOW 4      /* more than INT_MAX tile instances */
#define GSR_ERR_PREFILTERED 5   /* prefiltered=1 but a point failed the frustum test */

/* Scratch allocation callback: return a device pointer to at least `nbytes`
 * bytes that stays valid until the matching backward call has returned.
 * Replaces std::function<char*(size_t)> (rasterize_points.cu:29-43). */
typedef void* (*gsr_alloc_fn)(void* ctx, size_t nbytes);

/* Argument structs.  gsr_rasterize_forward and gsr_rasterize_backward each take one struct; the Gaussians
 * (gsr_scene) and the camera (gsr_view) are grouped, because both passes read them.  A caller zero-initialises
 * the struct, sets struct_size to its sizeof and assigns the fields it uses by name: an optional pointer left
 * NULL selects the call without it, as documented on the field.  A struct_size other than the library's own
 * sizeof is GSR_ERR_ARGUMENT (the message names both sizes), checked before any other field is read. */

/* The Gaussians: what the forward renders and the backward differentiates. */
typedef struct gsr_scene {
    int P; /* Gaussians */
    int D; /* active SH degree, 0..3; (D + 1)^2 coefficients must be present.  Ignored with colors_precomp */
    int M; /* SH coefficients per Gaussian in shs: all of them (dc NULL) or the REST (dc given; 15 at
              degree 3).  0 if shs is NULL */
    const float* means3D; /* [P,3] */
    /* Separate-DC layout: the 3DGS-accel rasterizer's interface (the build that ships SparseGaussianAdam), which
     * the reference's callers select with separate_sh=True (train.py:41-45,105,144;
     * gaussian_renderer/__init__.py:106-125 passes dc= and shs= = GaussianModel._features_dc / _features_rest).
     * dc [P,1,3] is coefficient 0; the colour is the same polynomial as with one combined [P,M+1,3] array.
     * NULL: the combined layout, shs holding all M coefficients; dL_ddc is then not written. */
    const float* dc;
    const float* shs;            /* [P,M,3]; NULL with colors_precomp, or with dc when M == 0 */
    const float* colors_precomp; /* [P,3] or NULL: colours from SH (then dc or shs, and view.campos, are required) */
    const float* opacities;      /* [P] */
    const float* scales;         /* [P,3]; NULL with cov3D_precomp */
    float scale_modifier;
    const float* rotations;     /* [P,4]; NULL with cov3D_precomp */
    const float* cov3D_precomp; /* [P,6] or NULL: covariance from scales and rotations */
} gsr_scene;

/* The camera and the image. */
typedef struct gsr_view {
    int width, height;
    const float* background; /* [3] */
    const float* viewmatrix; /* [16], read column-major */
    const float* projmatrix; /* [16], read column-major */
    const float* campos;     /* [3]; the forward needs it for SH colours only (NULL with colors_precomp), the
                                backward always */
    float tan_fovx, tan_fovy;
    int antialiasing;
} gsr_view;

/* Forward pass (CudaRasterizer::Rasterizer::forward).  out_color, out_invdepth and radii are written for every
 * element.  With P == 0 nothing is launched or allocated and the two results are 0. */
typedef struct gsr_forward_args {
    size_t struct_size; /* sizeof(gsr_forward_args) */
    gsr_scene scene;
    gsr_view view;
    /* the three scratch buffers (see "Conventions" above); pass them back unchanged to the backward */
    gsr_alloc_fn geom_alloc;
    void* geom_ctx;
    gsr_alloc_fn binning_alloc; /* called again, with a larger size, when capacity_hint was too small */
    void* binning_ctx;
    gsr_alloc_fn image_alloc;
    void* image_ctx;
    int prefiltered; /* != 0: GSR_ERR_PREFILTERED if a point fails the frustum test */
    int debug;       /* != 0: synchronise and check for errors after every stage */
    void* stream;
    float* out_color;    /* [3,H,W] */
    float* out_invdepth; /* [1,H,W] */
    int* radii;          /* [P] */
    /* > 0: no mid-forward host synchronisation.  The binning buffer is requested for capacity_hint instances
     * before the count is known (typically the previous call's num_rendered plus a margin), the tile sort runs
     * on that capacity with the unused slots padded, and the host waits once, for the instance count only.  If
     * num_rendered exceeds the hint, the binning stage is redone exactly (gsr_forward_rebuilds counts these).
     * <= 0: the reference's synchronising forward -- the count is read back (CR/rasterizer_impl.cu:313) before
     * the binning buffer is requested. */
    int capacity_hint;
    /* results, written by the call */
    int num_rendered; /* (tile, Gaussian) instances: the backward's R */
    /* The capacity the binning buffer was laid out for: num_rendered or capacity_hint, whichever is larger,
     * rounded up to a multiple of 256 instances -- over which the buffer's size determines the layout, so the
     * backward can take binning_bytes instead of this value.  Only a capacity whose rounding would pass INT_MAX
     * is kept exact (C = num_rendered); the backward still recovers that layout from the buffer's size. */
    int binning_capacity;
} gsr_forward_args;

/* Backward pass (CudaRasterizer::Rasterizer::backward), of the forward that filled the three buffers, with that
 * forward's scene and view.  Every element of every non-NULL output is written (no pre-zeroing needed).  The
 * backward also sets the gradient records' content bytes, which live in the forward's binning buffer (zeroed
 * by the forward); they depend on the geometry only, so a second backward of the same forward (retain_graph)
 * sets the same bytes.  With P == 0 nothing is launched. */
typedef struct gsr_backward_args {
    size_t struct_size; /* sizeof(gsr_backward_args) */
    gsr_scene scene;
    gsr_view view;
    int R;            /* the forward's num_rendered */
    const int* radii; /* [P], as the forward wrote them */
    void* geom_buffer;
    void* binning_buffer; /* may be NULL when R == 0 */
    void* image_buffer;
    /* The binning buffer's layout: binning_capacity is the value the forward returned, or 0.  With 0 and a
     * nonzero binning_bytes (the buffer's size) the capacity is recovered from the size: the forward lays the
     * buffer out for a multiple of 256 instances, over which the size determines the layout (so the buffer can
     * travel through any tensor copy, e.g. saved-tensor hooks), or, for a capacity above INT_MAX - 255, exactly
     * for R, which the size identifies too.  With 0 and 0 the layout is the exact one for R.  A size that
     * matches no layout, or a given capacity whose layout has another size, is GSR_ERR_ARGUMENT. */
    int binning_capacity;
    size_t binning_bytes;
    /* upstream gradients */
    const float* dL_dpix;       /* [3,H,W] */
    const float* dL_dinvdepths; /* [1,H,W] or NULL: no inverse-depth loss; dL_dinvdepth must then be NULL too */
    /* [1,H,W] or NULL (then exactly the call without it): the gradient of the accumulated alpha A
     * (gsr_render_alpha).  dA/dalpha_i = +final_T / (1 - alpha_i) has the form of the colour's background term
     * (CR/backward.cu:587-590) with -1 in place of bg . dL_dpix, and enters the blend backward there; the
     * conventions are the colour's (no gradient through the early termination, the skip tests or the 0.99
     * clamp).  Every output carries the alpha loss's share except dL_dcolor / dL_dsh / dL_ddc / dL_dinvdepth,
     * which it does not reach.  gsr_camera_backward, run on the outputs, gives the camera gradients of the alpha
     * loss too (campos gets none: A does not depend on the colours).  Not supported yet: a gradient for the
     * background. */
    const float* dL_dalphas;
    /* outputs */
    float* dL_dmean2D; /* [P,3] */
    /* [P,3] or NULL (then exactly the call without it): the absolute screen-space gradient, the densification
     * statistic of AbsGS (gsplat's absgrad).  dL_dmean2D is a signed sum over pixels, so the per-pixel terms of
     * a large Gaussian cancel across its centre; the absolute value has to be taken per pixel, inside the render
     * backward.  For Gaussian g
     *     dL_dmean2D_abs[g] = (sum_pix |t_x(g, pix)|, sum_pix |t_y(g, pix)|, 0),
     * t_x, t_y the terms the reference adds per pixel into dL_dmean2D (CR/backward.cu:600-601), in the same NDC
     * units (x 0.5 W, 0.5 H).  A pixel's term is its total over all upstream maps (colour, inverse depth and,
     * when given, alpha), the sum runs over every tile instance of the Gaussian, and the skip tests, early
     * termination, 0.99 clamp and antialiasing are those of dL_dmean2D.  Every element is written; rows with
     * radii == 0 are zero, and R == 0 gives zeros.  Every other output is what the call without it writes
     * (bitwise on the record path, "bwd_atomic" 0, where dL_dmean2D_abs is bitwise reproducible too).
     * GSR_ERR_ARGUMENT when the census is set (gsr_census_set): the census form of the render backward has no
     * absolute-gradient variant; and with view_block: view blocks carry no absolute gradient. */
    float* dL_dmean2D_abs;
    float* dL_dconic;    /* [P,4] or NULL: not stored (gsr_camera_backward reads it) */
    float* dL_dopacity;  /* [P] */
    float* dL_dcolor;    /* [P,3] */
    float* dL_dinvdepth; /* [P] or NULL, together with dL_dinvdepths */
    float* dL_dmean3D;   /* [P,3] */
    float* dL_dcov3D;    /* [P,6] */
    float* dL_ddc;       /* [P,1,3]; required with scene.dc (and SH colours), not written without it */
    float* dL_dsh;       /* [P,M,3]; required with scene.shs (and SH colours) */
    float* dL_dscale;    /* [P,3]; required with scene.scales, as dL_drot */
    float* dL_drot;      /* [P,4] */
    /* NULL: the whole backward, into the outputs above.  Non-NULL (device, 16-byte aligned,
     * gsr_view_block_floats(P) floats): the screen-space backward of the multi-GPU view exchange (below) -- the
     * backward up to the per-Gaussian sums (CR/backward.cu:433-612 = renderCUDA backward), written with the
     * camera into the block; the per-Gaussian backward is left to gsr_gauss_backward_views and the outputs above
     * are ignored.  Colours come from SH (dc + shs, or shs alone) and cov3D from scales / rotations:
     * colors_precomp or cov3D_precomp with a view block is GSR_ERR_ARGUMENT, as is dL_dmean2D_abs.  Not
     * covered: an alpha loss over view blocks (the view exchange sets no dL_dalphas).  dL/dmeans2D of this view
     * is the block's float pair at [64 + 4P + 2g] (densification). */
    float* view_block;
    int debug; /* != 0: synchronise and check for errors after every stage */
    /* 48 bytes per tile instance for the per-instance gradient records, plus 40 bytes and a live-list slot per
     * Gaussian */
    gsr_alloc_fn scratch_alloc;
    void* scratch_ctx;
    void* stream;
} gsr_backward_args;

int gsr_rasterize_forward(gsr_forward_args* args);
int gsr_rasterize_backward(const gsr_backward_args* args);

/* Accumulated alpha (silhouette): a third differentiable map beside colour and inverse depth,
 * A[pix] = 1 - final_T[pix], final_T the transmittance after the pixel's last contributor -- the
 * factor of the background in out_color (CR/forward.cu:497-505).  A pixel no Gaussian reaches has
 * A == 0.0 exactly.  No reference counterpart; the forward keeps final_T in its image buffer anyway.
 *
 * gsr_render_alpha: writes A ([1,H,W], row-major, every element) from the image buffer of a finished
 *   forward of the same width and height, one small kernel on `stream`; call it after the forward, on the
 *   forward's stream or one ordered behind it.  Valid only for P > 0 (a forward of no Gaussians allocates no
 *   image buffer: A is then all zeros).  GSR_ERR_ARGUMENT on non-positive sizes or a NULL pointer.
 * Its gradient enters the backward as gsr_backward_args.dL_dalphas. */
int gsr_render_alpha(int width, int height, const void* image_buffer, float* out_alpha, void* stream);

/* Per-Gaussian contribution statistics (importance pruning: LightGaussian's global significance, RadSplat's
 * max-blend-weight pruning, visibility-count prunes).  The blend weight of Gaussian g at pixel pix is
 * w(g, pix) = alpha(g, pix) T(g, pix), the factor of g's colour in out_color (CR/forward.cu:484-489).  A
 * (Gaussian, pixel) pair contributes iff the forward blended it: alpha >= 1/255, power <= 0, and the pair lies
 * before the pixel's termination -- the pairs the backward forms a gradient term for.  The maximum and the count
 * cannot be had from any backward (autograd only sees sums), so they are formed by a pass of their own.
 *
 * gsr_contrib_stats: from the three buffers of a finished forward (under every option, with or without a capacity
 *   hint, also one no backward will follow; P, R, width, height, binning_capacity / binning_bytes as
 *   gsr_backward_args takes them) into stats ([P,4], device, 16-byte aligned), row g =
 *     weight_sum    f32       sum of w over g's contributing pixels
 *     weight_max    f32       max of w over them
 *     pixel_count   u32 bits  their number
 *     weighted_sum  f32       sum of w m(pix), m = pixel_weight ([H,W] row-major); 0 when pixel_weight is NULL
 *   accumulate == 0: every row is written; rows of culled or never-blended Gaussians are zero, and P == 0 or
 *   R == 0 gives zeros (P == 0 launches nothing and the buffers may be NULL; R == 0 needs only stats).
 *   accumulate != 0: rows are combined with what they hold -- sums and counts add, the maximum maxes -- so one
 *   buffer accumulates any number of views with no extra pass; the caller zeroes it first.  Counts wrap at 2^32.
 *   weight_max and pixel_count do not depend on summation order and are bitwise reproducible; the two sums add
 *   each tile instance's share with float atomics, in the hardware's order.  The call reads the forward's
 *   buffers and writes only stats: a backward of the same forward, before or after it, is unaffected, and it may
 *   be repeated.  It runs on `stream`, which must be the forward's or ordered behind it.  Not differentiable.  The
 *   census (gsr_census_set) does not apply and the stage profiler does not time the call.  Multi-GPU: each rank
 *   computes its views' rows; all-reduce the four columns with SUM, MAX, SUM, SUM.
 *   GSR_ERR_ARGUMENT on negative or zero sizes, a NULL or misaligned stats, missing buffers with R > 0, or a
 *   binning buffer whose size matches no layout for R. */
int gsr_contrib_stats(int P, int R, int width, int height, const void* geom_buffer, const void* binning_buffer,
                      const void* image_buffer, int binning_capacity, size_t binning_bytes,
                      const float* pixel_weight /* [H,W] row-major or NULL */, int accumulate,
                      float* stats /* [P,4], 16-byte aligned */, void* stream);

/* N-channel feature rendering (semantic / language feature fields, latent appearance codes, normals, ids: gsplat's
 * N-D features).  Per-Gaussian feature vectors F [P,C] (float32, any C >= 1) are blended per pixel with the weights
 * the forward used for the colour, w(g, pix) = alpha(g, pix) T(g, pix) over the (pixel, Gaussian) pairs of
 * gsr_contrib_stats:
 *     Fmap[c, pix] = sum_g w(g, pix) F[g, c]                 (no background term, no clamp)
 * A pass of its own over a finished forward's buffers instead of ceil(C/3) renders with colors_precomp, each of which
 * would repeat preprocess, binning and the sort.
 *
 * gsr_render_features: from the three buffers of a finished forward (under every option, with or without a capacity hint,
 *   also one no backward will follow, and copies of the buffers; P, R, width, height, binning_capacity /
 *   binning_bytes as gsr_backward_args takes them) and features ([P,C], device) into out_features
 *   ([C,H,W], device), every element written; a pixel no Gaussian reaches is 0.0 exactly, and P == 0 or R == 0 gives
 *   zeros (the buffers may then be NULL).  The weights depend on the forward's discrete state alone (list order,
 *   blend masks, last contributors), each pixel is written by one wave and nothing is added atomically: the map is
 *   bitwise reproducible, and the same bits after a half-tile, a whole-tile ("fwd_quads" 4) or a no_backward
 *   forward.  Read-only on the buffers and repeatable; a backward of the colour before or after it is unaffected.
 *   Runs on `stream`, which must be the forward's or ordered behind it.  The census and the stage profiler do not
 *   apply.  GSR_ERR_ARGUMENT on C <= 0 (or more than 65535 chunks of gsr_render_features_chunk() channels),
 *   negative or zero sizes, NULL pointers, missing buffers with R > 0, or a binning buffer whose size matches no
 *   layout for R.
 * gsr_render_features_backward: the backward of that map for the upstream gradient dL_dout_features ([C,H,W]).
 *   Writes every element of dL_dfeatures ([P,C]): dL_dF[g, c] = sum_pix w(g, pix) U[c, pix], zero rows for Gaussians
 *   that never blended.  With view_block != NULL (gsr_view_block_floats(P) floats, 16-byte aligned) it also forms
 *   the geometry part: with s_g(pix) = sum_c U[c, pix] F[g, c],
 *     dL/dalpha_g(pix) = T_g s_g - (sum_{h behind g} w_h s_h) / (1 - alpha_g),
 *   the suffix sum had front to back from out_features (the forward's map, an input), then the render backward's
 *   chain to the per-Gaussian sums of dL/dmean2D, dL/dopacity and dL/dconic, written as a view block of this loss
 *   alone: colour and inverse-depth sums zero, flag words from radii and the geometry buffer's SH clamp flags, the
 *   header from viewmatrix, projmatrix, campos, tan_fovx / tan_fovy and antialiasing.  gsr_gauss_backward_views with
 *   n_views = 1 turns it into dL/dmeans3D, dL/dopacity, dL/dscales, dL/drotations (its SH outputs are zero: pass a
 *   zero dc with M = 0); dL/dmeans2D is the first two floats of row g of the block's second sum array, at float
 *   64 + 4 P + 4 g.  Conventions are the colour's: no gradient through skips, termination or the 0.99 clamp.
 *   view_block == NULL (frozen geometry): only dL_dfeatures, and out_features, the camera, radii and the scratch
 *   callback are not used.  scratch_alloc provides 64 bytes per Gaussian plus a bit each with a view block.
 *   Per-Gaussian sums are added with float atomics, in the hardware's order: not bitwise reproducible.
 *   Not covered: the feature loss does not reach the camera tensors or the absolute gradient, features have no
 *   background, the multi-GPU view exchange is not wired, and precomputed cov3D gets no feature geometry gradient
 *   (gsr_gauss_backward_views needs scales and rotations).
 * gsr_render_features_chunk: channels one wave blends at once (the kernels' channel chunk). */
int gsr_render_features(int P, int C, int R, int width, int height, const void* geom_buffer,
                        const void* binning_buffer, const void* image_buffer, int binning_capacity,
                        size_t binning_bytes, const float* features /* [P,C] */, float* out_features /* [C,H,W] */,
                        void* stream);
int gsr_render_features_backward(int P, int C, int R, int width, int height, const void* geom_buffer,
                                 const void* binning_buffer, const void* image_buffer, int binning_capacity,
                                 size_t binning_bytes, const float* features, const float* out_features,
                                 const float* dL_dout_features, float* dL_dfeatures /* [P,C] */,
                                 float* view_block /* or NULL */, const float* viewmatrix, const float* projmatrix,
                                 const float* campos, float tan_fovx, float tan_fovy, int antialiasing,
                                 const int* radii, gsr_alloc_fn scratch_alloc, void* scratch_ctx, void* stream);
int gsr_render_features_chunk(void);

/* Depth-distortion map (the Mip-NeRF 360 distortion regulariser as 2DGS, GOF, RaDe-GS, PGSR and gsplat's distloss use
 * it): a per-pixel quantity QUADRATIC in the blend weights, which no choice of features can give.  t [P] (float32) is
 * a per-Gaussian scalar of the caller's choice (view depth, 1/z, a contracted distance).  For a pixel let 1..n be its
 * contributing entries in the forward's list order, front to back -- the (pixel, Gaussian) pairs of gsr_contrib_stats
 * with the weights w_i = alpha_i T_i the forward used:
 *     D = 2 sum_i w_i (t_i A_{i-1} - B_{i-1}),    A_k = sum_{j<=k} w_j,    B_k = sum_{j<=k} w_j t_j
 * the ordered form 2 sum_{i behind j} w_i w_j (t_i - t_j) (gsplat's convention, one front-to-back pass).  It equals
 * sum_{i,j} w_i w_j |t_i - t_j| whenever t is non-decreasing along the list (any increasing function of view depth);
 * for other t it is the SIGNED form.  No background term.
 *
 * gsr_render_distortion: from the three buffers of a finished forward (as gsr_render_features takes them, under the
 *   same conditions) and t into out_distortion ([H,W]) and out_moments ([2,H,W], which the backward takes as input:
 *   A_n of every pixel and its B_n taken about the pixel's first contributor, sum_i w_i (t_i - t_1) -- D depends on
 *   differences of t only, and the kernels work in that frame so that float32 loses nothing to the size of t itself),
 *   every element written; a pixel no Gaussian reaches is 0.0 exactly, and P == 0 or R == 0
 *   gives zeros (the buffers may then be NULL).  Each pixel is written by one wave, nothing is added atomically: the
 *   map is bitwise reproducible, and the same bits after a half-tile, a whole-tile or a no_backward forward and for
 *   copies of the buffers.  Read-only on the buffers and repeatable.  Argument rules and error codes are
 *   gsr_render_features' (with C = 1).
 * gsr_render_distortion_backward: the backward of that map for the upstream gradient dL_dout_distortion ([H,W]).
 *   Writes every element of dL_dt ([P]): with the prefix sums taken BEFORE entry i,
 *     dD/dt_i = 2 w_i (2 A_prev + w_i - A_n).
 *   With view_block != NULL it also forms the geometry part: with g_i = dD/dw_i = 2 (t_i (2 A_prev - A_n) + B_n -
 *   2 B_prev) and sum_h w_h g_h = 2 D (D is homogeneous of degree 2 in w),
 *     dL/dalpha_i = U (T_i g_i - (2 D - sum_{h<=i} w_h g_h) / (1 - alpha_i)),
 *   then exactly gsr_render_features_backward's chain and outputs: a view block of this loss alone for
 *   gsr_gauss_backward_views, the same use of the camera, radii and the scratch callback, the same conventions (no
 *   gradient through skips, termination or the 0.99 clamp), the same things not covered.  view_block == NULL (only
 *   t needs a gradient): dL_dt alone, and out_distortion, the camera, radii and the scratch callback are not used.
 *   Per-Gaussian sums are added with float atomics, in the hardware's order: not bitwise reproducible. */
int gsr_render_distortion(int P, int R, int width, int height, const void* geom_buffer, const void* binning_buffer,
                          const void* image_buffer, int binning_capacity, size_t binning_bytes,
                          const float* t /* [P] */, float* out_distortion /* [H,W] */,
                          float* out_moments /* [2,H,W] */, void* stream);
int gsr_render_distortion_backward(int P, int R, int width, int height, const void* geom_buffer,
                                   const void* binning_buffer, const void* image_buffer, int binning_capacity,
                                   size_t binning_bytes, const float* t, const float* out_distortion,
                                   const float* out_moments, const float* dL_dout_distortion, float* dL_dt /* [P] */,
                                   float* view_block /* or NULL */, const float* viewmatrix, const float* projmatrix,
                                   const float* campos, float tan_fovx, float tan_fovy, int antialiasing,
                                   const int* radii, gsr_alloc_fn scratch_alloc, void* scratch_ctx, void* stream);

/* Per-pixel selections from the blend weights: WHICH Gaussian a pixel "is".  Every other per-pixel output is a sum
 * over the weights; these are arg-selects over them, which no feature map and no autograd graph can give.  For a
 * pixel let 1..n be its contributing entries in the forward's list order -- the (pixel, Gaussian) pairs of
 * gsr_contrib_stats: blended, before termination, below the pixel's n_contrib -- T_i the transmittance BEFORE entry
 * i is blended (T_1 = 1) and w_i = alpha_i T_i.
 *   Median contributor m: the LAST contributor with T_m > 0.5 (2DGS's rule, `if (T > 0.5) { median_depth = depth;
 *     median_contributor = ...; }` evaluated before T is updated): the contributor that takes T from above one half
 *     to at most one half, or the pixel's last contributor when T never gets there.  median_ids[pix] is m's Gaussian
 *     index (int32) and median[pix] = t[m], a COPY of the caller's per-Gaussian scalar t [P] (float32; view depth for
 *     the median depth, conventions as gsr_render_distortion's t).  A pixel with no contributor: id -1, value 0.0.
 *   Top-K, 1 <= K <= gsr_render_select_max_k() (8): the K contributors of largest w in descending w; on equal w the
 *     earlier one in list order ranks first (a later entry displaces only on strict >).  topk_ids [K,H,W] int32 and
 *     topk_weights [K,H,W] float32; ranks beyond the pixel's contributor count hold id -1 and weight 0.0.
 * No background term.  Each pixel is written once by the wave that owns it, nothing is added atomically: all four
 * outputs are bitwise reproducible, and the same bits after a half-tile, a whole-tile ("fwd_quads" 4) or a
 * no_backward forward and for copies of the buffers.  The expected depth invdepth / alpha blurs across depth
 * discontinuities; the median does not, and is meant to be used beside the distortion map of the same render.
 *
 * gsr_render_select: from the three buffers of a finished forward (as gsr_render_features takes them, under the same
 *   conditions; argument rules and error codes are gsr_render_features' with C = 1) in ONE pass for both selections.
 *   t, out_median and out_median_ids are all set or all NULL (no median); K in 0 .. max and out_topk_ids,
 *   out_topk_weights set exactly when K > 0; K == 0 without the median is GSR_ERR_ARGUMENT.  Every element of the
 *   outputs given is written.  P == 0 or R == 0 fills ids with -1 and floats with 0 (the buffers, and with P == 0
 *   t, may then be NULL).  Read-only on the buffers and repeatable; a backward of the colour before or after it is
 *   unaffected.
 * gsr_render_select_max_k: the largest K this build supports.
 * gsr_render_median_backward: dL_dt[g] = sum over the pixels with median_ids[pix] == g of dL_dout_median[pix]
 *   ([H,W]); every element of dL_dt ([P]) is written (zeroed, then added into with float atomics in the hardware's
 *   order: NOT bitwise reproducible); ids outside 0 .. P-1 are skipped.  The median is piecewise constant in the
 *   blend weights, so there is no geometry gradient (2DGS forms none either): t is its only differentiable input, and
 *   the gradient reaches the geometry through whatever t was computed from.  The ids and the top-K outputs are not
 *   differentiable (gsr_render_features blends differentiably).  P == 0 does nothing. */
int gsr_render_select(int P, int R, int width, int height, const void* geom_buffer, const void* binning_buffer,
                      const void* image_buffer, int binning_capacity, size_t binning_bytes,
                      const float* t /* [P] or NULL */, int K, float* out_median /* [H,W] or NULL */,
                      int* out_median_ids /* [H,W] or NULL */, int* out_topk_ids /* [K,H,W] or NULL */,
                      float* out_topk_weights /* [K,H,W] or NULL */, void* stream);
int gsr_render_select_max_k(void);
int gsr_render_median_backward(int P, int width, int height, const int* median_ids /* [H,W] */,
                               const float* dL_dout_median /* [H,W] */, float* dL_dt /* [P] */, void* stream);

/* Multi-GPU view exchange (gaussian_splatting_amd/distributed.py
 * ViewExchange).  The reference trains on one GPU; sharding views over N ranks needs the
 * N views' parameter gradients summed on every rank.  Instead of all-reducing the 59-float
 * parameter gradients (2 (N-1)/N x 236 B per Gaussian per rank over xGMI), each rank
 * all-gathers the other ranks' "view blocks" -- a camera header and, per Gaussian, the 10
 * summed render gradients (dL/dcolour, dL/dinvdepth, dL/dmean2D, dL/dopacity, dL/dconic)
 * plus a visibility / SH-clamp word, 44 B -- and every rank runs the per-Gaussian backward
 * over all views at once (10 (N-1) floats received per Gaussian instead of 118 (N-1)/N).
 *
 * gsr_view_block_floats(P): floats in one view block (padded to 256 B).
 * gsr_rasterize_backward with gsr_backward_args.view_block set: the screen-space backward, which
 *   writes this rank's view block (documented on the field).
 * gsr_gauss_backward_views: the rest of the backward (CR/backward.cu:153-429,
 *   computeCov2DCUDA + preprocessCUDA, as gsr_rasterize_backward's last stage) for all
 *   n_views gathered blocks (blocks[v * block_floats ...]), writing the SUM over views of
 *   dL/dmeans3D, dL/ddc, dL/dsh, dL/dopacity, dL/dscales, dL/drotations.  With one view it
 *   equals the single-view backward bit for bit. */
unsigned long long gsr_view_block_floats(int P);

int gsr_gauss_backward_views(int P, int D, int M, const float* means3D, const float* dc, const float* shs,
                             const float* opacities, const float* scales, const float* rotations, float scale_modifier,
                             int n_views, const float* blocks, long long block_floats, float* dL_dmean3D,
                             float* dL_ddc, float* dL_dsh, float* dL_dopacity, float* dL_dscale, float* dL_drot,
                             void* stream);

/* Sparse view blocks.  Behind saturated pixels most Gaussians get no render gradient (about
 * 14% of a 1M@1080p view have one), so a view block travels packed: its header (64 floats,
 * the entry count as uint32 bits in float 63) and, per Gaussian that is visible with a non-zero
 * sum, 12 floats (index bits, the 10 sums, the flag word), in Gaussian order.
 * gsr_view_pack_floats(n): floats of a packed block holding n entries (padded to 256 B).
 * gsr_view_pack_scratch_bytes(P): device scratch gsr_view_block_pack needs.
 * gsr_view_block_pack: view_block (gsr_view_block_floats(P) floats) -> packed
 *   (gsr_view_pack_floats(cap) floats); *count (device uint32, may be NULL) receives the entry
 *   count, which may exceed cap (then only the first cap entries are written).
 * gsr_view_block_unpack: n_views packed blocks (packed_floats apart) -> n_views dense view
 *   blocks (gsr_view_block_floats(P) apart), entries beyond cap ignored.  Only the flag words
 *   are cleared first: a Gaussian left out has flag 0 and its sums are left as they were
 *   (gsr_gauss_backward_views never reads them).  Unpacked blocks give gsr_gauss_backward_views
 *   the dense blocks' result (a Gaussian left out had all-zero sums, which add nothing). */
unsigned long long gsr_view_pack_floats(long long entries);
unsigned long long gsr_view_pack_scratch_bytes(int P);
int gsr_view_block_pack(int P, const float* view_block, float* packed, long long cap, void* scratch,
                        unsigned int* count, void* stream);
/* Chunked exchange (distributed.py ViewExchange(chunks=K), no reference counterpart): the same over the
 * Gaussians [g0, g1) only -- one chunk's packed block (entries keep their absolute index), so chunk k+1's
 * all-gather can run while the multi-view backward works on chunk k.  gsr_view_block_pack(...) is
 * gsr_view_block_pack_range(P, 0, P, ...). */
int gsr_view_block_pack_range(int P, int g0, int g1, const float* view_block, float* packed, long long cap,
                              void* scratch, unsigned int* count, void* stream);
int gsr_view_block_unpack(int P, int n_views, const float* packed, long long packed_floats, float* blocks,
                          long long cap, void* stream);

/* Packed mode of the multi-view backward (what ViewExchange uses): no dense blocks are rebuilt.
 * gsr_view_block_index: flags ([n_views][P] uint32) cleared, then for entry i of packed block v,
 *   flags[v * P + g] = i << 4 | the entry's flag bits (cap < 2^28 entries).  One 4-byte store per
 *   entry instead of the unpack's 44 bytes scattered over four arrays.
 * gsr_gauss_backward_views_packed: gsr_gauss_backward_views over the packed blocks themselves
 *   (camera from each packed header, sums from the entry its flag word indexes); the same result
 *   as over the unpacked blocks. */
int gsr_view_block_index(int P, int n_views, const float* packed, long long packed_floats, unsigned int* flags,
                         long long cap, void* stream);
/* Chunk form: clears and sets the flags of Gaussians [g0, g1) only (the packed blocks hold that chunk). */
int gsr_view_block_index_range(int P, int g0, int g1, int n_views, const float* packed, long long packed_floats,
                               unsigned int* flags, long long cap, void* stream);
int gsr_gauss_backward_views_packed(int P, int D, int M, const float* means3D, const float* dc, const float* shs,
                                    const float* opacities, const float* scales, const float* rotations,
                                    float scale_modifier, int n_views, const float* packed, long long packed_floats,
                                    const unsigned int* flags, float* dL_dmean3D, float* dL_ddc, float* dL_dsh,
                                    float* dL_dopacity, float* dL_dscale, float* dL_drot, void* stream);

/* Live-list form (sparse outputs): only the Gaussians some view flags are visited.
 * gsr_views_live_floats(P): uint32 words of the list buffer (entries + shard counters).
 * gsr_views_live_list: builds it from the flags of gsr_view_block_index.
 * gsr_gauss_backward_views_live: gsr_gauss_backward_views_packed over the listed Gaussians only,
 *   one lane each; every output row of the others is left untouched, so the caller zeroes the
 *   outputs beforehand (ViewExchange does it on a second stream while the all-gather runs). */
unsigned long long gsr_views_live_floats(int P);
int gsr_views_live_list(int P, int n_views, const unsigned int* flags, unsigned int* live, void* stream);
/* Chunk form: only Gaussians [g0, g1) are listed. */
int gsr_views_live_list_range(int P, int g0, int g1, int n_views, const unsigned int* flags, unsigned int* live,
                              void* stream);
int gsr_gauss_backward_views_live(int P, int D, int M, const float* means3D, const float* dc, const float* shs,
                                  const float* opacities, const float* scales, const float* rotations,
                                  float scale_modifier, int n_views, const float* packed, long long packed_floats,
                                  const unsigned int* flags, const unsigned int* live, float* dL_dmean3D,
                                  float* dL_ddc, float* dL_dsh, float* dL_dopacity, float* dL_dscale, float* dL_drot,
                                  void* stream);

/* Camera-pose gradients (no reference counterpart: the reference's rasterizer treats the camera as a
 * constant).  Run after gsr_rasterize_backward of the same forward, on the same stream, with that
 * call's inputs and five of its per-Gaussian outputs: dL_dmean2D [P,3], dL_dconic [P,4] (which that call must
 * then be given; 16-byte aligned), dL_dopacity [P], dL_dcolor [P,3] and dL_dinvdepth [P] (NULL if the backward
 * had none).  Rows of Gaussians with radii == 0 are not read.  geom_buffer is the forward's geometry buffer
 * (its SH clamp flags are read); width / height are the forward's.  Colours as in the forward: dc + shs (M
 * rest coefficients), shs alone (dc NULL), or colors_precomp (then dc, shs, D, M and campos are ignored).
 * Writes every element of
 *   dL_dviewmatrix [16]  entry k belongs to viewmatrix[k] as the forward reads it; entries 3, 7, 11, 15 (the
 *                        last column, never read) are zero;
 *   dL_dprojmatrix [16]  likewise; entries 2, 6, 10, 14 (the depth column, never read) are zero;
 *   dL_dcampos     [3]   zero with precomputed colours;
 * and P == 0 gives zeros.  The three tensors are independent inputs, as the forward reads them: viewmatrix
 * feeds the view-space point (cov2D's Jacobian, the inverse depth) and cov2D's rotation, projmatrix the screen
 * position, campos the SH view direction.  Conventions are dL_dmean3D's: no gradient through culling, the
 * radius, the tile rectangle, skips or termination; a clamped view-space x / y is a constant in the Jacobian;
 * with antialiasing the reference's formula for dL/dcov2D, not the derivative of its forward.
 * No atomics: for the same per-Gaussian inputs the outputs are the same bit for bit.  scratch_alloc provides
 * 128 bytes per 1024 Gaussians. */
int gsr_camera_backward(int P, int D, int M, int width, int height, const float* means3D, const float* dc,
                        const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                        float scale_modifier, const float* rotations, const float* cov3D_precomp,
                        const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                        float tan_fovy, const int* radii, const void* geom_buffer, const float* dL_dmean2D,
                        const float* dL_dconic, const float* dL_dopacity, const float* dL_dcolor,
                        const float* dL_dinvdepth, int antialiasing, gsr_alloc_fn scratch_alloc, void* scratch_ctx,
                        void* stream, float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos);

/* Frustum test, view-space z > 0.2 (CudaRasterizer::Rasterizer::markVisible).
 * `present` is P bytes (bool). */
int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     unsigned char* present, void* stream);

/* Inspection of a forward's private state, for parity tests (the reference keeps the same
 * state in its binning / image buffers: BinningState::point_list and ImageState::ranges /
 * n_contrib / accum_alpha, cuda_rasterizer/rasterizer_impl.h:39-72).  Copies, on `stream`,
 * device to device, into caller-provided device arrays (any may be NULL to skip it):
 *   ranges     [tiles][2]  each tile's [start, end) in point_list (identifyTileRanges);
 *   point_list [R]         the tile lists, tile-major, each tile in (depth, index) order;
 *                          entry = Gaussian index << 4 | the forward's 4-bit quadrant mask;
 *   n_contrib  [H*W]       last contributor (1-based list position) per pixel;
 *   final_T    [H*W]       transmittance after the last contributor.
 * binning_capacity / binning_bytes as in gsr_backward_args. */
int gsr_debug_forward_state(int P, int width, int height, int R, int binning_capacity, size_t binning_bytes,
                            const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                            unsigned int* ranges, unsigned int* point_list, unsigned int* n_contrib, float* final_T,
                            void* stream);

/* Inspection of the reachable-prefix sort ("sort_prefix" option): copies, on `stream`, device to
 * device, the number of entries of each tile's list in final order (sorted_len [tiles]; the whole
 * length unless K4 sorted only a prefix) and the number of tiles the forward redid because a wave
 * passed the sorted prefix (redo_count [1]).  Either pointer may be NULL. */
int gsr_debug_sort_state(int P, int width, int height, const void* geom_buffer, unsigned int* sorted_len,
                         unsigned int* redo_count, void* stream);
/* Near-first binning state of a forward (the "near_mass" option; tests): the depth bin of its cut
 * (0xffffffff: none -- off, or the frame's opacity mass never reached the target) and, when there was a
 * cut, each tile's near entries [start, start + near) as K4 sorted them ([tiles][2] uint32). */
int gsr_debug_near_state(int P, int width, int height, const void* geom_buffer, unsigned int* zcut,
                         unsigned int* near_ranges, void* stream);

/* Number of forwards (process-wide) whose capacity hint was too small, so the binning stage
 * was redone with the exact count (gsr_forward_args.capacity_hint). */
long long gsr_forward_rebuilds(void);

/* Host-side statistics since the last reset (reset != 0 clears after reading), for finding time
 * the GPU spends waiting on the host.  values[0..8] = for (a) the forwards' waits for their
 * instance count (the one host synchronisation of a forward, CR/rasterizer_impl.cu:313; here an
 * event behind the binning count), (b) whole forward calls, (c) whole backward calls: the number of
 * calls, their total host time in ms and the longest one in ms.  Up to n values are written. */
int gsr_host_stats(double* values, int n, int reset);

/* Runtime options (no reference counterpart): the library's alternative kernel paths, readable
 * and settable in-process so that every path it ships is parity-tested (tests/test_gpu_options.py).
 * Each default comes from the environment variable GSR_<NAME> (upper case) at first use.
 *   "fused_bin"  1|0    capacity-mode binning with the tile scan folded into the scatter (forward)
 *   "fwd_quads"  2|4    8x8 quadrants per forward wave: half tiles | whole tiles
 *   "bwd_seg_ck" 1..2^20 backward work unit length in 256-entry checkpoints; read by the forward, which
 *                        writes the units and records the value for its backward (a backward always
 *                        walks the segments its own forward made, whatever the option is by then)
 *   "host_total" 1|0    the binning kernels store num_rendered into mapped host memory | a copy is queued
 *   "zero_fill"  3|1|2|0 dense backward outputs zero-filled by extra blocks of render_bwd's launch
 *                        (default) | on a side stream | on the launch stream before gauss_bwd | not at
 *                        all (gauss_bwd writes every row)
 *   "live_list"  1|0    gauss_bwd over the list of Gaussians with a render gradient | a lane per Gaussian
 *                        (only with zero_fill != 0)
 *   "sort_prefix" L|0   (L in 1..1024) when the frame's mean list length is at least 2 L: of the lists longer than
 *                        1024 entries sort only the first L (+ the rest of a bucket), the part the blend
 *                        reaches, and redo the rare tile whose walk passes it | sort whole lists
 *                        (default L = 1024)
 *   "count_wait" 2|1|0  capacity-hinted forwards: no event behind the instance count, the host polls the
 *                        mapped count slot the binning kernel stores into (spins 100 us, then yields the
 *                        core between polls) | polls the event recorded behind the count (20 ms at most,
 *                        then blocks) | blocks in hipEventSynchronize (woken by the completion interrupt)
 *   "bwd_grid"   0|1|2  render_bwd's grid: 2 blocks per tile, each walking units i, i + G, ... when the
 *                        grid sized for the shortest segments would be over 4x that (5M@4K) | that worst-case
 *                        grid, one unit per block | always the strided grid
 *   "bwd_atomic" 0|1    the render backward writes one gradient record per (tile, Gaussian) instance, summed
 *                        per Gaussian by gauss_reduce in a fixed order: bitwise deterministic | adds
 *                        each instance's ten sums into per-Gaussian rows with float atomics (no records, no
 *                        gauss_reduce; the order of the adds follows the hardware: default, 1M@1080p -1.5 µs,
 *                        5M@4K -104 µs per step).  Read by the forward,
 *                        which zeroes the rows when it is 1 and marks its geometry buffer; a backward takes
 *                        the atomic path iff the option is 1 and its geometry buffer carries that mark (a
 *                        buffer from a forward without the option, or one copied in, gets the record path).
 *                        A forward with the option also skips the record path's inputs (record starts,
 *                        content bits); a record-path backward of its buffer writes them first.
 *                        The screen-space backward (view blocks) follows the same rule: its block's sums
 *                        come from the rows (gauss_live_views) instead of gauss_reduce
 *   "near_mass"  M|0    near-first binning (capacity-hinted forwards with the fused scan): only the Gaussians
 *                        in front of the depth at which the screen-averaged opacity mass (the integral of
 *                        alpha over the plane, summed front to back, over the image area) reaches M get keys
 *                        and are sorted; a tile whose forward walk passes its near entries is redone with its
 *                        whole list, so every output is the whole lists' (default M = 30; a pixel saturates
 *                        at 9.2) | every instance keyed and sorted
 *   "touched_run" 0|N   the atomic backward's per-Gaussian pass: one workgroup lists the touched Gaussians of
 *                        128 x N consecutive ones (N a power of two up to 32; others round down) and runs
 *                        their backward 128 at a time | 0: by the frame -- N = 16 where the mean tile list holds
 *                        2048 entries or more (few Gaussians touched: 5M@4K), else 1 (default)
 * Every option is read once per forward / backward call, so a concurrent gsr_option_set never splits
 * one call's launches between two values.
 * gsr_option_get returns -1 for an unknown name; gsr_option_set returns GSR_ERR_ARGUMENT for an
 * unknown name or an out-of-range value.  Not synchronised against calls running on other threads. */
int gsr_option_set(const char* name, int value);
int gsr_option_get(const char* name);
/* The same options for calls made on THIS thread only, over the process-wide values (e.g. a forward that no
 * backward will follow: "bwd_atomic" 0 skips zeroing the atomic backward's accumulator rows -- a backward of
 * it then takes the record path).  gsr_option_get reports the value in force on the calling thread.
 * gsr_option_clear_thread(name) drops one override, (NULL) all of them.  Errors as gsr_option_set. */
int gsr_option_set_thread(const char* name, int value);
int gsr_option_clear_thread(const char* name);

/* Forget what the library recorded about a geometry buffer's last forward (whether its accumulator rows were
 * zeroed and its record inputs written).  A buffer the library did not write at that address -- a copy, one
 * restored from a checkpoint -- must be forgotten before its backward, which then writes the record inputs
 * and takes the deterministic record path.  (The Python layer calls it for any geometry tensor that is not
 * the one its forward returned.)  Always GSR_OK. */
int gsr_geom_forget(const void* geom_buffer);

/* Message of the last error on this thread ("" if none). */
const char* gsr_last_error(void);

/* Library version string, e.g. "gsr 0.1.0 gfx950". */
const char* gsr_version(void);

/* The build's input hash: sha256 (hex) over every source, header and compiler flag the library was
 * compiled from (gaussian_splatting_amd/build.py input_hash), compiled into the library.  The loader
 * compares it with the hash of the tree it runs from, so a library built from other sources is
 * detected instead of used (no reference counterpart). */
const char* gsr_build_id(void);

/* Per-stage device timing with hipEvents recorded on the launch stream.
 * stage_mask selects the stages to time (bit s = stage s, -1 = all, 0 = off);
 * each timed stage adds one event pair to the stream (~10 us of idle GPU per
 * event on gfx950, so time only what you need inside a measured region).
 * collect() waits for the recorded events and adds their elapsed times to
 * running per-stage totals; it returns the number of stages and fills up to
 * max_stages totals (ms) and call counts.  Stage names come from
 * gsr_profile_stage_name(). */
int gsr_profile_enable(int stage_mask);
int gsr_profile_collect(double* total_ms, long long* calls, int max_stages);
void gsr_profile_reset(void);
const char* gsr_profile_stage_name(int stage);

/* Census (diagnostic; no reference counterpart): with a device buffer of 10 zeroed uint64
 * counters set, the render kernels of later forward / backward calls run their census
 * instantiations (slower: a few extra wave-uniform ops per evaluation) and add, per call:
 *   [0] forward list entries staged (per half-tile wave; each tile's two halves both stage)
 *   [1] forward (entry, 8x8 quadrant) evaluations  (64 pixel evaluations each)
 *   [2] forward (pixel, entry) pairs with alpha > 0 reaching a live pixel
 *   [3] forward (pixel, entry) pairs blended (alpha > 0 and the pixel does not end there)
 *   [4] backward list entries staged
 *   [5] backward (entry, quadrant) evaluations
 *   [6] backward (pixel, entry) pairs with a gradient term (alpha > 0, before n_contrib)
 *   [7] backward per-entry wave reductions (gradient records with content)
 *   [8] backward evaluations in which no pixel has a gradient term (idle)
 *   [9] forward evaluations in which no pixel blends (idle)
 * NULL turns the census off.  Not thread-safe against concurrent calls. */
int gsr_census_set(void* device_counters);

#ifdef __cplusplus
}
#endif

#endif /* GSR_H_INCLUDED */
