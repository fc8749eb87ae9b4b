/*
 * gsrast.h -- C ABI of the MI355X-native differentiable Gaussian rasterizer.
 *
 * This is the drop-in boundary for the hot path that pomelyu/gaussian_splatting_lightning reaches
 * through `diff_gaussian_rasterization` (reference call sites:
 *   gs_lightning/lightning/gs_lightning_module.py:322-348   GaussianRasterizationSettings + GaussianRasterizer
 *   scripts/render_trained_image.py:98-124                  inference call, means2D=None
 *   tests/rasterizer_python/test_mark_visible.py:13-14      GaussianRasterizer(s).markVisible(points)).
 * The submodule that normally implements it (graphdeco-inria/diff-gaussian-rasterization@dr_aa,
 * .gitmodules:1-4) is not vendored; each entry point below replaces one of its pybind exports
 * (`_C.rasterize_gaussians`, `_C.rasterize_gaussians_backward`, `_C.mark_visible`, SURVEY.md §2.1 and
 * §8(b)).  Signatures are plain C: device pointers, sizes and a hipStream_t passed as void*.  No torch
 * types cross this boundary; the Python host layer (gaussian_splatting_lightning_amd/rasterizer.py)
 * binds it with ctypes.
 *
 * Conventions (identical to the reference's torch API):
 *   means3D (P,3), opacities (P,1), scales (P,3), rotations (P,4) as (w,x,y,z), shs (P,M,3),
 *   colors_precomp (P,3), cov3D_precomp (P,6) upper triangle, viewmatrix / projmatrix (4,4) row-major
 *   in the row-vector convention (p_view = [p,1] @ V), campos (3), background (3);
 *   out_color (3,H,W), out_invdepth (1,H,W), radii (P) int32.
 * All pointers are DEVICE pointers (fp32, contiguous) unless stated; every launch goes on `stream`.
 * Return value: 0 on success, nonzero error code; gsr_last_error() gives the message.
 */
#ifndef GSRAST_H
#define GSRAST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Scratch buffers are owned by the caller and grown through this callback, mirroring the
 * reference's resizeFunctional() lambdas over uint8 torch tensors (notes/rasterizer_note.h:27-40).
 * `which` is one of GSR_BUF_*; the callback returns a device pointer to >= nbytes bytes that stays
 * valid until the caller frees it (the forward's three buffers must survive until the backward). */
typedef char *(*gsr_alloc_fn)(void *ctx, int which, size_t nbytes);

enum {
    GSR_BUF_GEOM = 0,
    GSR_BUF_BINNING = 1,
    GSR_BUF_IMAGE = 2,
    GSR_BUF_BWD_SCRATCH = 3,
    GSR_BUF_CAMERA_PARTIALS = 4, /* gsr_backward, only when a camera gradient is asked for; free after the call */
    GSR_BUF_BACKGROUND_PARTIALS = 5, /* gsr_backward_ext, only when dL_dbackground is asked for; free after the call */
    GSR_BUF_CONTRIB_SCRATCH = 6 /* gsr_contributions (gsr_contrib_scratch_bytes); free after the call */
};

enum {
    GSR_OK = 0,
    GSR_ERR_ARG = 1,      /* invalid shape/pointer/option (RuntimeError in Python) */
    GSR_ERR_HIP = 2,      /* HIP runtime error */
    GSR_ERR_ALLOC = 3,    /* allocation callback returned NULL */
    GSR_ERR_OVERFLOW = 4, /* more than 2^32-1 tile instances */
    GSR_ERR_UNSUPPORTED = 5
};

typedef struct gsr_forward_args {
    int P;                        /* number of Gaussians */
    int D;                        /* active SH degree (0..3) */
    int M;                        /* SH coefficients stored per Gaussian (shs.size(1)), 0 if none */
    int W, H;                     /* image size */
    const float *background;      /* (3) */
    const float *means3D;         /* (P,3) */
    const float *colors_precomp;  /* (P,3) or NULL (then shs is required) */
    const float *opacities;       /* (P) */
    const float *scales;          /* (P,3) or NULL (then cov3D_precomp is required) */
    float scale_modifier;
    const float *rotations;       /* (P,4) or NULL */
    const float *cov3D_precomp;   /* (P,6) or NULL */
    const float *viewmatrix;      /* (16) */
    const float *projmatrix;      /* (16) */
    const float *campos;          /* (3) */
    float tan_fovx, tan_fovy;
    const float *shs;             /* (P,M,3) or NULL */
    int prefiltered;              /* accepted; the frustum test is applied either way */
    int antialiasing;             /* EWA 2D filter opacity compensation (dr_aa) */
    int debug;                    /* synchronise + check after every stage */
    float *out_color;             /* (3,H,W) */
    float *out_invdepth;          /* (H,W) or NULL */
    int *radii;                   /* (P) */
    int64_t num_big_out;          /* OUTPUT: Gaussians with > 64 instances (pass to gsr_backward) */
} gsr_forward_args;

/* Replaces `_C.rasterize_gaussians` (rasterize_points.cu RasterizeGaussiansCUDA -> Rasterizer::forward).
 * Runs preprocess, depth sort, scan, one device->host read of the instance count, tile expansion,
 * tile sort, range identification and compositing.  *num_rendered receives the instance count. */
int gsr_forward(gsr_forward_args *args, gsr_alloc_fn alloc, void *alloc_ctx, void *stream,
                int64_t *num_rendered);

typedef struct gsr_backward_args {
    int P, D, M, W, H;
    int64_t R;                    /* num_rendered returned by gsr_forward */
    int64_t num_big;              /* num_big_out returned by gsr_forward, or < 0: read from geom_buffer on the device
                                     (the upstream backward signature does not carry it; gsr_torch_ext.cpp) */
    const float *background;
    const float *means3D;
    const float *colors_precomp;  /* or NULL */
    const float *opacities;
    const float *scales;          /* or NULL */
    float scale_modifier;
    const float *rotations;       /* or NULL */
    const float *cov3D_precomp;   /* or NULL */
    const float *viewmatrix, *projmatrix, *campos;
    float tan_fovx, tan_fovy;
    const float *dL_dpix;         /* (3,H,W) */
    const float *dL_dinvdepth;    /* (H,W) or NULL */
    const float *shs;             /* or NULL */
    const int *radii;             /* (P) from the forward */
    char *geom_buffer, *binning_buffer, *image_buffer; /* from the forward */
    int antialiasing, debug;
    /* outputs, each fully written (no pre-zeroing needed); any may be NULL to skip it */
    float *dL_dmeans2D;           /* (P,3), z = 0, NDC units (pixel grad * (W/2, H/2)) */
    float *dL_dcolors;            /* (P,3) */
    float *dL_dopacity;           /* (P) */
    float *dL_dmeans3D;           /* (P,3) */
    float *dL_dcov3D;             /* (P,6) */
    float *dL_dsh;                /* (P,M,3); may be NULL only when dL_dcolors_sh is given */
    float *dL_dscales;            /* (P,3) */
    float *dL_drotations;         /* (P,4) */
    /* (P,3) colour gradient with computeColorFromSH's clamp mask applied, i.e. the factor that multiplies
     * the SH basis in dL/dsh.  With dL_dsh == NULL this is the compact per-view SH gradient that
     * gsr_sh_backward_views expands (multi-view data parallelism); NULL to skip. */
    float *dL_dcolors_sh;
    /* (P,2) densification statistics of this view (gaussian_model.py:175-181): [i][0] = |dL/dmeans2D[i][:2]|,
     * [i][1] = 1 if radii[i] > 0 else 0; NULL to skip. */
    float *densify_stats;
    /* densify_accumulate != 0: densify_stats += this view's statistics instead of =, i.e. the reference's
     * add_densification_stats (xyz_gradient_accum += norm, denom += 1 for visible Gaussians) across views and
     * steps; max_radii2D (P) int32, if non-NULL, becomes max(max_radii2D, radii) (gaussian_model.py:175-176). */
    int densify_accumulate;
    int *max_radii2D;
    /* Split backward, so a gradient exchange can overlap the per-Gaussian stage (multiview.py; no counterpart in
     * the reference, whose batch is one view):
     *   stages = GSR_BWD_ALL (0): everything in one call;
     *   GSR_BWD_COMPOSITE: the compositing backward and the big-Gaussian reduction only -- the per-instance gradient
     *     rows land in the GSR_BUF_BWD_SCRATCH buffer, which the caller keeps for the next calls; no output written;
     *   GSR_BWD_GAUSSIANS: the per-Gaussian stage only, over Gaussians [g_begin, g_end), reading the rows from
     *     bwd_scratch (the GSR_BWD_COMPOSITE call's buffer).  Every output pointer then addresses Gaussian
     *     g_begin's row (a slice of a full array, or a chunk-sized buffer).
     * g_begin = g_end = 0 means the whole range [0, P) (any stage). */
    int stages;
    int64_t g_begin, g_end;
    char *bwd_scratch;
    /* Camera block of the multi-view exchange (multiview.py), written by the per-Gaussian stage so that no extra
     * launch is needed: campos_rows (campos_nrows, 3) gets campos in row campos_rank and zeros in the others (a
     * SUM all-reduce of the block then yields every rank's camera).  NULL to skip. */
    float *campos_rows;
    int campos_rank, campos_nrows;
    /* Camera gradients (GSR_ABI_VERSION 3), each NULL to skip and fully written otherwise: those of viewmatrix,
     * projmatrix and campos as three independent inputs, in their own row-major layout.
     *   dL_dviewmatrix (16): column 3 is zero (p_view = [p,1] @ V reads columns 0-2); the view-space point and the
     *     rotation inside the EWA covariance projection both contribute.  Outside the 1.3 tan(fov) clamp of the EWA
     *     Jacobian the clamp is differentiated as written (autograd's result), whereas dL_dmeans3D keeps the upstream
     *     backward's convention there (the clamped coordinate taken as constant);
     *   dL_dprojmatrix (16): column 2 is zero (the 2D mean reads x, y, w; depth comes from viewmatrix);
     *   dL_dcampos (3): minus the sum of the SH view-direction term of dL_dmeans3D (zero with colors_precomp or M = 0).
     * Sums over the Gaussians in a fixed order (per-wave partials in the caller's GSR_BUF_CAMERA_PARTIALS buffer, then
     * a two-level tree whose shape depends only on the Gaussian range): no float atomics, bitwise reproducible.
     * GSR_BWD_ALL writes the whole sums, GSR_BWD_GAUSSIANS those over [g_begin, g_end) (the caller adds the chunks),
     * GSR_BWD_COMPOSITE ignores them; with P = 0 they are zero. */
    float *dL_dviewmatrix, *dL_dprojmatrix, *dL_dcampos;
} gsr_backward_args;

enum { GSR_BWD_ALL = 0, GSR_BWD_COMPOSITE = 1, GSR_BWD_GAUSSIANS = 2 };

/* Replaces `_C.rasterize_gaussians_backward` (RasterizeGaussiansBackwardCUDA -> Rasterizer::backward).
 * Deterministic: per-tile gradient rows are reduced in fixed order (no float atomics). */
int gsr_backward(const gsr_backward_args *args, gsr_alloc_fn alloc, void *alloc_ctx, void *stream);

/* Rendered alpha, a per-pixel background and the background's gradients: a side struct of gsr_forward_ext /
 * gsr_backward_ext, versioned by its own size like gsr_state_layout (fields are only appended; the library reads the
 * fields past the caller's struct_size as NULL), so gsr_forward_args / gsr_backward_args and GSR_ABI_VERSION stay as
 * they are.  With T_final the transmittance the forward leaves behind a pixel's last contributor:
 *   out_alpha = 1 - T_final (0 on a pixel no Gaussian reaches);
 *   out_color_c = C_c + T_final * background_image_c(pix): args->background's expression with the pixel's own value
 *     (an image whose every pixel is the vector gives the vector's bits);
 *   backward: the per-pixel scalar that carries the background through the reverse walk starts from
 *     sum_c B_c(pix) dL_dpix_c(pix) - dL_dalpha(pix); nothing else of the walk changes;
 *   dL_dbackground_image_c(pix) = T_final(pix) * dL_dpix_c(pix) (one rounding);
 *   dL_dbackground_c = the sum of that over the pixels, in a fixed tree whose shape depends only on (W, H): per-workgroup
 *     partials in the caller's GSR_BUF_BACKGROUND_PARTIALS buffer, then one fixed-order pass (no float atomics, bitwise
 *     reproducible).
 * background_image and dL_dalpha are read, and the two gradients written, by GSR_BWD_ALL and GSR_BWD_COMPOSITE;
 * GSR_BWD_GAUSSIANS ignores the struct.  With P = 0 (or nothing rendered) T_final = 1: alpha 0, colour the background,
 * the gradients dL_dpix and its sums. */
typedef struct gsr_composite_ext {
    size_t struct_size;               /* sizeof as the caller was built; fields past it are read as NULL */
    const float *background_image;    /* (3,H,W) or NULL; when given it replaces args->background (which may then be NULL) */
    float *out_alpha;                 /* forward: (H,W), fully written, or NULL */
    const float *dL_dalpha;           /* backward: (H,W) or NULL */
    float *dL_dbackground;            /* backward: (3), fully written, or NULL */
    float *dL_dbackground_image;      /* backward: (3,H,W), fully written, or NULL */
} gsr_composite_ext;
/* gsr_forward / gsr_backward are these with ext = NULL.  GSR_ERR_ARG, before any device call or allocation, when
 * neither args->background nor ext->background_image is given or struct_size ends before the first pointer field. */
int gsr_forward_ext(gsr_forward_args *args, const gsr_composite_ext *ext, gsr_alloc_fn alloc, void *alloc_ctx,
                    void *stream, int64_t *num_rendered);
int gsr_backward_ext(const gsr_backward_args *args, const gsr_composite_ext *ext, gsr_alloc_fn alloc, void *alloc_ctx,
                     void *stream);

/* Absolute screen-space gradients for densification (AbsGS; `absgrad` in gsplat): a second side struct, versioned by
 * its own size like gsr_composite_ext, so gsr_backward_args, gsr_composite_ext and GSR_ABI_VERSION stay as they are.
 *   dL_dmeans2D_abs[i] = (sum_pix |m_x(i,pix)|, sum_pix |m_y(i,pix)|), m(i,pix) being what pixel pix adds to
 *     dL_dmeans2D[i][:2] in the compositing backward under every upstream gradient of the call (colour, inverse depth,
 *     gsr_composite_ext's dL_dalpha and background), in dL_dmeans2D's units.  The signed sum lets the contributions of
 *     a Gaussian that is too bright on one side and too dark on the other cancel; this one does not.  Exactly 0 for a
 *     Gaussian that is culled or that no pixel takes.  Summed in the fixed order of the other gradients (no float
 *     atomics): two calls give the same bits, and every other output keeps the bits it has without this struct.
 *   densify_abs != 0: args->densify_stats[i][0] is formed from this vector instead of from dL_dmeans2D[i][:2], as
 *     sqrt(x * x + y * y) with each operation rounded once; [i][1], densify_accumulate and max_radii2D are unchanged.
 *     GSR_ERR_ARG, before any device work, without args->densify_stats or without dL_dmeans2D_abs.
 * Stages: the rows are produced by GSR_BWD_ALL and GSR_BWD_COMPOSITE whenever dL_dmeans2D_abs is non-NULL (the
 * composite-only call does not write through it: the pointer is the request), into a GSR_BUF_BWD_SCRATCH buffer of
 * gsr_bwd_scratch_bytes_abs bytes; GSR_BWD_ALL and GSR_BWD_GAUSSIANS write the output, the latter for Gaussians
 * [g_begin, g_end) through a pointer that addresses Gaussian g_begin's row, from the scratch buffer of a composite call
 * that was given the struct (with the same num_big).  With P = 0 nothing is written. */
typedef struct gsr_absgrad_ext {
    size_t struct_size;       /* sizeof as the caller was built; fields past it are read as NULL / 0 */
    float *dL_dmeans2D_abs;   /* (P,2), fully written, or NULL */
    int densify_abs;          /* densify_stats[:,0] from the absolute sums */
} gsr_absgrad_ext;
/* gsr_backward / gsr_backward_ext are this with absgrad = NULL (and ext = NULL). */
int gsr_backward_abs(const gsr_backward_args *args, const gsr_composite_ext *ext, const gsr_absgrad_ext *absgrad,
                     gsr_alloc_fn alloc, void *alloc_ctx, void *stream);

/* Per-Gaussian feature channels (the arbitrary-channel `colors` of gsplat): a third side struct, versioned by its own
 * size like the two above, so gsr_forward_args, gsr_backward_args, gsr_composite_ext, gsr_absgrad_ext and
 * GSR_ABI_VERSION stay as they are.  features (P,C), 1 <= C <= 64, any fp32 values (semantic or language features,
 * normals, view-space depth, ids, ...), are composited with the weights of the colour render:
 *   out_features_c(pix) = sum_i w_i(pix) features[i][c],  w_i = alpha_i T_i, front to back like the colour, with NO
 *     background term (fully written; zeros where no Gaussian reaches).  The weights are replayed from the state the
 *     colour composite recorded, with its arithmetic: the same values passed as colours (background 0) give the same bits.
 *   backward: dL_dfeatures[i][c] = sum_pix w_i(pix) dL_dout_features_c(pix) (fully written; exactly 0 for a Gaussian
 *     that is culled or that no pixel takes), and, through alpha, the features' share of EVERY other gradient of the
 *     call: their geometry terms are added into the per-instance gradient rows before the per-Gaussian stage, so
 *     dL_dmeans2D / dL_dopacity / dL_dmeans3D / dL_dcov3D / dL_dscales / dL_drotations, densify_stats and the camera
 *     gradients come out as the joint gradient of colour, inverse depth, alpha and features.  Summed in a fixed order
 *     (no float atomics): two calls give the same bits.
 *   dL_dout_features == NULL: none of the feature work is launched, dL_dfeatures (if given) is written as zeros and
 *     every other output keeps the bits it has without the struct.
 * The pointers need only be 4-B aligned (a row of (P,C) with odd C is not 16-B aligned).
 * With P = 0 or nothing rendered out_features is zeros and dL_dfeatures is written as zeros (nothing for P = 0).
 * Scratch: the backward asks for a GSR_BUF_BWD_SCRATCH buffer of gsr_bwd_scratch_bytes_features(R, num_big, C) bytes:
 * gsr_bwd_scratch_bytes plus the feature rows of ONE channel block (R x 8 floats for C <= 8, else R x 16 floats; the
 * blocks of 8 / 16 channels are walked and gathered one after the other and reuse them) plus one such row per big
 * Gaussian -- 64 B per instance at most, whatever C is, instead of 4 C.
 * GSR_ERR_ARG, before any device work or allocation: C < 1 or C > 64, a missing features (P > 0) / out_features
 * pointer, struct_size ending before the first pointer field.
 * GSR_ERR_UNSUPPORTED, before any device work -- not yet built:
 *   features together with gsr_absgrad_ext.dL_dmeans2D_abs (|.| is not linear: the absolute sums of a joint call
 *     cannot be formed by adding the features' terms);
 *   features with stages != GSR_BWD_ALL (the split backward).
 * Under the "guard" tuning knob the feature kernels take the guard's decision path (guard_alpha_pass) like the colour
 * kernels: supported, provided forward and backward run with the same knob, as for the colour. */
typedef struct gsr_features_ext {
    size_t struct_size;               /* sizeof as the caller was built; fields past it are read as NULL */
    int C;                            /* channels, 1..64 */
    const float *features;            /* (P,C) */
    float *out_features;              /* forward: (C,H,W), fully written */
    const float *dL_dout_features;    /* backward: (C,H,W) or NULL */
    float *dL_dfeatures;              /* backward: (P,C), fully written, or NULL */
} gsr_features_ext;
/* gsr_forward_ext / gsr_backward_abs are these with feat = NULL. */
int gsr_forward_features(gsr_forward_args *args, const gsr_composite_ext *ext, const gsr_features_ext *feat,
                         gsr_alloc_fn alloc, void *alloc_ctx, void *stream, int64_t *num_rendered);
int gsr_backward_features(const gsr_backward_args *args, const gsr_composite_ext *ext, const gsr_absgrad_ext *absgrad,
                          const gsr_features_ext *feat, gsr_alloc_fn alloc, void *alloc_ctx, void *stream);

/* Depth distortion map: the Mip-NeRF 360 distortion loss per pixel (2DGS's and gsplat's distloss), a fourth side
 * struct versioned by its own size, so every other struct and GSR_ABI_VERSION stay as they are.  Over the pairs the
 * colour forward composited (sorted index below the pixel's contributor count, the composite's alpha decision; under
 * the "guard" knob the guarded one), with the colour render's weights w_i = alpha_i T_i and a per-Gaussian depth t_i:
 *   out_distortion(pix) = sum_i sum_j w_i w_j |t_i - t_j|    (no background term; exactly 0 where no Gaussian reaches)
 *   map GSR_DISTORTION_Z:   t = z, the view-space depth whose inverse out_invdepth composites;
 *   map GSR_DISTORTION_NDC: t = far / (far - near) * (1 - near / z), 2DGS's bounded mapping (near_plane, far_plane).
 * Tile lists are sorted by view depth and both maps are non-decreasing in z, so it is evaluated in one pass as
 * 2 sum_i w_i (t_i A_<i - M_<i) with the prefix sums A_<i = sum_(j<i) w_j and M_<i = sum_(j<i) w_j t_j.
 *   forward: out_distortion, total_weight (sum_i w_i) and total_moment (sum_i w_i t_i), (H,W) each, fully written.  The
 *     two totals are state: the backward needs them as the forward left them.  Every other output of the call keeps
 *     the bits it has without the struct.
 *   backward: dL_ddistortion (H,W) enters, through the weights and through t, EVERY gradient of the call (dL_dmeans2D /
 *     dL_dopacity / dL_dmeans3D / dL_dcov3D / dL_dscales / dL_drotations, densify_stats, the camera gradients): its
 *     geometry terms and its depth term are added into the per-instance gradient rows before the per-Gaussian stage, in
 *     a fixed order (no float atomics): two calls give the same bits.  It needs no scratch beyond gsr_bwd_scratch_bytes
 *     (or gsr_bwd_scratch_bytes_features with features).
 *   dL_ddistortion == NULL: none of the distortion work is launched and every output keeps the bits it has without the
 *     struct.
 * With P = 0 or nothing rendered the three maps are zeros.  Together with gsr_features_ext in one call: supported, both
 * add into the same rows, one launch after the other.
 * GSR_ERR_ARG, before any device work or allocation: an unknown map; with GSR_DISTORTION_NDC near_plane <= 0 or
 * far_plane <= near_plane (or either not a number); a missing out_distortion (forward) / total_weight / total_moment
 * pointer; struct_size ending before the first pointer field.
 * GSR_ERR_UNSUPPORTED, before any device work -- not built: distortion together with gsr_absgrad_ext.dL_dmeans2D_abs,
 * and with stages != GSR_BWD_ALL (the split backward). */
enum { GSR_DISTORTION_Z = 0, GSR_DISTORTION_NDC = 1 };
typedef struct gsr_distortion_ext {
    size_t struct_size;               /* sizeof as the caller was built; fields past it are read as NULL */
    int map;                          /* GSR_DISTORTION_Z or GSR_DISTORTION_NDC */
    float near_plane;                 /* GSR_DISTORTION_NDC: > 0 */
    float far_plane;                  /* GSR_DISTORTION_NDC: > near_plane */
    float *out_distortion;            /* forward: (H,W), fully written */
    float *total_weight;              /* (H,W): written by the forward, read by the backward */
    float *total_moment;              /* (H,W): written by the forward, read by the backward */
    const float *dL_ddistortion;      /* backward: (H,W) or NULL */
} gsr_distortion_ext;
/* gsr_forward_features / gsr_backward_features are these with dist = NULL. */
int gsr_forward_distortion(gsr_forward_args *args, const gsr_composite_ext *ext, const gsr_features_ext *feat,
                           const gsr_distortion_ext *dist, gsr_alloc_fn alloc, void *alloc_ctx, void *stream,
                           int64_t *num_rendered);
int gsr_backward_distortion(const gsr_backward_args *args, const gsr_composite_ext *ext,
                            const gsr_absgrad_ext *absgrad, const gsr_features_ext *feat,
                            const gsr_distortion_ext *dist, gsr_alloc_fn alloc, void *alloc_ctx, void *stream);

/* Median depth map: per pixel the view depth and the id of the Gaussian at which the ray's transmittance crosses 1/2
 * (2DGS's depth_ratio = 1 surface, the depth its TSDF mesh extraction fuses), a fifth side struct versioned by its own
 * size, so every other struct and GSR_ABI_VERSION stay as they are.  Over the pairs the colour forward composited, front
 * to back (sorted index below the pixel's contributor count, the composite's alpha decision; under the "guard" knob the
 * guarded one), with T carried from 1 as T <- T (1 - alpha): pair i is selected while the T reaching it exceeds 0.5, so
 * the median is the last contributor whose incoming transmittance exceeds 1/2, and the last contributor at all on a
 * pixel that never becomes half opaque.  A selection along the walk, not a weighted sum: no feature channel renders it.
 *   forward: out_median_depth (H,W) the selected Gaussian's view depth (the float the preprocess computed, copied),
 *     out_median_index (H,W) its id, median_pos (H,W) its position in the tile's sorted list; 0, -1 and -1 where no
 *     Gaussian reaches; all three fully written.  median_pos is state: the backward needs it as the forward left it,
 *     and it must be the plane the forward that built the call's geom / binning / image buffers wrote.  The library
 *     cannot tell a stale plane, or one of another forward on the same image size, from the right one: a position at
 *     or past the end of its tile's list is ignored (the walk stays in bounds), every other one is believed, and the
 *     gradients are then wrong without an error.
 *     Every other output of the call keeps the bits it has without the struct.
 *   backward: the selection is piecewise constant, so dL_dmedian_depth (H,W) reaches only the depth of the selected
 *     Gaussian, dL/dz_i = sum over the pixels whose median is i, and through z dL_dmeans3D and the camera gradients;
 *     opacities, scales, rotations, means2D and colours get nothing from it.  Summed per tile in a fixed order (no float
 *     atomics: two calls give the same bits) into the per-instance gradient rows before the per-Gaussian stage; it needs
 *     no scratch beyond gsr_bwd_scratch_bytes (or gsr_bwd_scratch_bytes_features with features).
 *   dL_dmedian_depth == NULL: none of the median backward is launched and every output keeps the bits it has without
 *     the struct.
 * With P = 0 or nothing rendered the planes are 0, -1, -1.  Together with gsr_features_ext and gsr_distortion_ext in one
 * call: supported.
 * GSR_ERR_ARG, before any device work or allocation: a missing out_median_depth / out_median_index (forward) or
 * median_pos pointer; struct_size ending before the first pointer field.
 * GSR_ERR_UNSUPPORTED, before any device work -- not built: the median together with gsr_absgrad_ext.dL_dmeans2D_abs,
 * and with stages != GSR_BWD_ALL (the split backward). */
typedef struct gsr_median_ext {
    size_t struct_size;               /* sizeof as the caller was built; fields past it are read as NULL */
    float *out_median_depth;          /* forward: (H,W), fully written */
    int32_t *out_median_index;        /* forward: (H,W), fully written */
    int32_t *median_pos;              /* (H,W): written by the forward, read by the backward */
    const float *dL_dmedian_depth;    /* backward: (H,W) or NULL */
} gsr_median_ext;
/* gsr_forward_distortion / gsr_backward_distortion are these with median = NULL. */
int gsr_forward_median(gsr_forward_args *args, const gsr_composite_ext *ext, const gsr_features_ext *feat,
                       const gsr_distortion_ext *dist, const gsr_median_ext *median, gsr_alloc_fn alloc,
                       void *alloc_ctx, void *stream, int64_t *num_rendered);
int gsr_backward_median(const gsr_backward_args *args, const gsr_composite_ext *ext, const gsr_absgrad_ext *absgrad,
                        const gsr_features_ext *feat, const gsr_distortion_ext *dist, const gsr_median_ext *median,
                        gsr_alloc_fn alloc, void *alloc_ctx, void *stream);

/* Per-Gaussian contribution statistics of one forward, for pruning and budgeting (LightGaussian's significance: the
 * sum; RadSplat: the max; Mini-Splatting / Taming-3DGS: the hit count; error-based densification: the sum under a
 * per-pixel error image).  Forward only: no gradient is involved.  GSR_ABI_VERSION and every other struct stay as they
 * are; this one is versioned by its own size like the ext structs.
 *   A pair (Gaussian i, pixel pix) CONTRIBUTES when the colour forward composited it: the pair test is the feature
 *   replay's (sorted index below the pixel's contributor count, the composite's alpha decision; under the "guard" knob
 *   the guarded one).  Its value is v = w_i(pix) = alpha_i T_i, the colour render's own weight, or with pixel_weights
 *   v = m(pix) * w_i(pix) as one fp32 product; a pixel whose m is not > 0 (zero, negative, NaN) is left out of
 *   everything.  Per Gaussian, over its contributing pairs with a pixel that is not left out:
 *     count[i] (int64) their number, wsum[i] the sum of v, wmax[i] the max of v (0 where there are none).
 *   All three are exactly 0 for a Gaussian that is culled or that no pixel takes; every element is written.
 *   accumulate != 0: count += , wsum = wsum + this view's sum (one fp32 add), wmax = max(wmax, this view's max), so a
 *   pass over views keeps one set of buffers.
 * The sums are formed in a fixed order (per instance inside its wave, then per Gaussian in instance order; no float
 * atomics): two calls give the same bits.  The call only reads the forward's three buffers: a gsr_backward on the same
 * state afterwards gives the bits it gives without it.  Scratch: one GSR_BUF_CONTRIB_SCRATCH buffer of
 * gsr_contrib_scratch_bytes(R, num_big) bytes through the callback (16 B per instance and per big Gaussian).
 * GSR_ERR_ARG, before any device work or allocation: every output NULL, a forward buffer (or radii) missing while
 * R > 0, struct_size ending before the first pointer field.  With P == 0 nothing is written; with R == 0 (everything
 * culled) the outputs are zeros, or under accumulate left as they are.  Launches go on `stream`, on its device. */
typedef struct gsr_contrib_args {
    size_t struct_size;            /* sizeof as the caller was built; fields past it are read as NULL / 0 */
    int P, W, H;
    int64_t R, num_big;            /* num_rendered and num_big_out of the forward (num_big < 0: read on the device) */
    const int32_t *radii;          /* (P) from the forward */
    const void *geom_buffer, *binning_buffer, *image_buffer; /* from the forward; only read */
    const float *pixel_weights;    /* (H,W) or NULL */
    int64_t *count;                /* (P) or NULL (not produced) */
    float *wsum, *wmax;            /* (P) each, or NULL */
    int accumulate;
} gsr_contrib_args;
size_t gsr_contrib_scratch_bytes(int64_t R, int64_t num_big);
int gsr_contributions(const gsr_contrib_args *args, gsr_alloc_fn alloc, void *alloc_ctx, void *stream);

/* Multi-view SH gradient from compact per-view factors (no counterpart in the reference, whose batch size is
 * one view: gs_lightning_module.py:139-141).  dL_dsh[g] = sum_v basis(normalize(means3D[g] - campos[v]))
 * (x) dL_dcolors_sh[v][g], i.e. the sum over views of gsr_backward's dL_dsh -- what an all-reduce of dL_dsh
 * computes, from 12 B per Gaussian per view instead of 12*M B.  campos (V,3), dL_dcolors_sh (V,P,3),
 * dL_dsh (P,M,3) fully written (coefficients above the active degree are zero).  Device pointers. */
int gsr_sh_backward_views(int P, int D, int M, int V, const float *means3D, const float *campos,
                          const float *dL_dcolors_sh, float *dL_dsh, void *stream);

/* The same expansion over factors gathered per Gaussian chunk (multiview.py's chunked exchange), in ONE launch:
 * dL_dcolors_sh is chunk-major -- chunk c covers Gaussians [c*chunk_len, min(P, (c+1)*chunk_len)) and is a
 * (V, L_c, 3) block at offset c*V*chunk_len*3.  chunk_len = 0 (or >= P) is gsr_sh_backward_views' (V,P,3). */
int gsr_sh_backward_views_chunked(int P, int D, int M, int V, int64_t chunk_len, const float *means3D,
                                  const float *campos, const float *dL_dcolors_sh, float *dL_dsh, void *stream);

/* Replaces `_C.mark_visible` (checkFrustum): present[i] = z_view(means3D[i]) > 0.2. */
int gsr_mark_visible(int P, const float *means3D, const float *viewmatrix, const float *projmatrix,
                     uint8_t *present, void *stream);

/* Fused SSIM loss -- replaces `fused_ssim(img1, img2, padding, train)` (rahul-goel/fused-ssim, imported at
 * gs_lightning_module.py:10 and used as 1 - fused_ssim(render, gt) at :100,279).  Images are (B,C,H,W)
 * contiguous fp32 device arrays; planes = B*C.  11x11 Gaussian window (sigma 1.5), C1 = 0.01^2, C2 = 0.03^2,
 * zero-padded "same" filtering; valid_padding = 1 averages only pixels >= 5 px from the border.
 * Forward: writes gsr_ssim_num_partials() partial sums of the SSIM map (mean = sum / counted pixels) and, when
 * the three derivative maps (planes*H*W each) are non-NULL, the per-pixel derivatives the backward needs.
 * Backward: dL_dimg1 from dL_dmean (device scalar: gradient of the mean SSIM) and the derivative maps.
 * GSR_ERR_ARG, before any device work, from both: planes outside [1, 65535], planes*H*W > 2^31 - 1, a NULL argument
 * (the forward's derivative maps: all given or all NULL), or valid_padding with H <= 10 or W <= 10 (no pixel counted). */
size_t gsr_ssim_num_partials(int planes, int H, int W);
int gsr_ssim_forward(int planes, int H, int W, const float *img1, const float *img2, int valid_padding,
                     float *partial_sums, float *dm_dmu1, float *dm_dsigma1_sq, float *dm_dsigma12, void *stream);
int gsr_ssim_backward(int planes, int H, int W, const float *img1, const float *img2, int valid_padding,
                      const float *dL_dmean, const float *dm_dmu1, const float *dm_dsigma1_sq,
                      const float *dm_dsigma12, float *dL_dimg1, void *stream);

/* Bilateral-grid colour correction (Wang et al., "Bilateral Guided Radiance Field Processing", SIGGRAPH 2024; the
 * layout of gsplat's lib_bilagrid).  grids is (num, 12, L, Gh, Gw) contiguous fp32 on the device: channel 4r + k of a
 * grid multiplies input colour k (k = 3: the offset) into output colour r.  image, out and the gradients of both are
 * (B, 3, H, W) contiguous fp32 on the device; grid_idx is a HOST array of B indices into [0, num): image b is sliced
 * through grid grid_idx[b].  Pixel (y, x) with value v samples its grid trilinearly (border-clamped) at
 *   ux = (x + 0.5) / W * (Gw - 1),  uy = (y + 0.5) / H * (Gh - 1),
 *   uz = clamp((0.299 v0 + 0.587 v1 + 0.114 v2) * (L - 1), 0, L - 1)
 * (a size-1 axis has coordinate 0) and out_r = A[4r] v0 + A[4r+1] v1 + A[4r+2] v2 + A[4r+3].
 * Backward: dL_dgrids (num grids, written whole: exact zeros for a grid no image selects; images that share a grid are
 * summed in image order; no atomics, so two calls give the same bits) and dL_dimage (through the affine, and through
 * uz where 0 < gray < 1); either may be NULL to skip it, and with both NULL the call does nothing and is GSR_OK.
 * dL_dgrids needs gsr_bilagrid_workspace_bytes(L, Gh, Gw, H, W) bytes of device workspace (one grid-sized slab per
 * split of a lattice column's pixel support; 0 when the support is not split: workspace may then be NULL).
 * Total variation: tv = (1 / num) sum over the three lattice axes of (the sum of squared first differences along the
 * axis) / (12 (n - 1) (the other two sizes)), an axis of size 1 contributing 0.  The forward writes
 * gsr_bilagrid_tv_num_partials() partial sums whose sum is tv; the backward writes dL_dgrids = dL_dtv[0] dtv/dgrids
 * (dL_dtv: device scalar).
 * GSR_ERR_ARG, before any device work: a NULL argument (other than the cases above), a non-positive num, L, Gh, Gw,
 * B, H or W, a grid index outside [0, num), 12 num L Gh Gw, H W or (2 max(H, W) + 1) max(Gh, Gw) above 2^31 - 1, or H
 * above 16 * 65535. */
size_t gsr_bilagrid_workspace_bytes(int L, int Gh, int Gw, int H, int W);
int gsr_bilagrid_slice_forward(int num, int L, int Gh, int Gw, const float *grids, int B, int H, int W,
                               const float *image, const int32_t *grid_idx, float *out, void *stream);
int gsr_bilagrid_slice_backward(int num, int L, int Gh, int Gw, const float *grids, int B, int H, int W,
                                const float *image, const int32_t *grid_idx, const float *dL_dout, float *dL_dgrids,
                                float *dL_dimage, void *workspace, void *stream);
size_t gsr_bilagrid_tv_num_partials(int num, int L, int Gh, int Gw);
int gsr_bilagrid_tv_forward(int num, int L, int Gh, int Gw, const float *grids, float *partial_sums, void *stream);
int gsr_bilagrid_tv_backward(int num, int L, int Gh, int Gw, const float *grids, const float *dL_dtv,
                             float *dL_dgrids, void *stream);

/* Fused Adam step over up to 16 parameter groups in one launch -- replaces the torch.optim.Adam(eps=1e-15)
 * step of the reference's six Gaussian parameter groups (gs_lightning_module.py:114-134).  All arrays are
 * contiguous fp32 device arrays of n elements, updated in place; step is the 1-based step count of each
 * group (torch keeps it per parameter).  No weight decay, no amsgrad, as configured by the reference. */
typedef struct gsr_adam_group {
    float *param;
    const float *grad;
    float *exp_avg, *exp_avg_sq;
    int64_t n;
    double lr;
    int64_t step;
} gsr_adam_group;
int gsr_adam_step(const gsr_adam_group *groups, int num_groups, double beta1, double beta2, double eps, void *stream);

/* Fused Adam step of the two SH parameter groups of a multi-view (one view per GPU) step, on the gradient that
 * gsr_sh_backward_views_chunked would expand -- sum_v basis(dir_v) (x) dL_dcolors_sh_v -- formed inside the update, so
 * the (P, M, 3) gradient is never written: features_dc (P, 1, 3) and features_rest (P, M - 1, 3) with their Adam
 * moments, updated in place with gsr_adam_step's arithmetic (each group with its own lr and 1-based step).  The
 * result is bitwise that of the expansion followed by gsr_adam_step.  M must be 16; V, chunk_len, means3D, campos and
 * dL_dcolors_sh as for gsr_sh_backward_views_chunked. */
typedef struct gsr_adam_sh_views_args {
    int P, D, M, V;
    int64_t chunk_len;
    const float *means3D, *campos, *dL_dcolors_sh;
    float *dc_param, *dc_exp_avg, *dc_exp_avg_sq;
    double dc_lr;
    int64_t dc_step;
    float *rest_param, *rest_exp_avg, *rest_exp_avg_sq;
    double rest_lr;
    int64_t rest_step;
    /* floats between consecutive Gaussians' rows of each parameter: 0 = packed ((P, 1, 3) / (P, M - 1, 3) tensors);
     * 48 = the two groups are the column blocks of ONE (P, 16, 3) tensor (dc_param = its base, rest_param = base + 3),
     * which the forward reads as shs without a concatenation.  The moments are always packed. */
    int64_t param_row_stride;
    /* the same for the moments: 0 = packed, 48 = exp_avg / exp_avg_sq are each one (P, 16, 3) tensor too (dc_* the
     * base, rest_* = base + 3).  With both at 48 every array is streamed as one coalesced run per 32 rows. */
    int64_t moment_row_stride;
} gsr_adam_sh_views_args;
int gsr_adam_sh_views_step(const gsr_adam_sh_views_args *a, double beta1, double beta2, double eps, void *stream);

/* The parameter activations the reference's GaussianModel puts in front of the rasterizer
 * (gs_lightning/modules/gaussian_model.py: get_scaling = exp(_scaling), get_opacity = sigmoid(_opacity),
 * get_rotation = torch.nn.functional.normalize(_rotation), i.e. q / max(|q|, 1e-12)) and their chain rule, so a
 * training step that keeps the raw parameters (what the optimizer steps) needs two launches instead of torch's
 * elementwise autograd graph.  Shapes: scaling / scales (N,3), opacity / opacities (N) or (N,1), rotation / rotations
 * (N,4); fp32 device arrays, the (N,4) ones 16-B aligned.  The backward takes the raw rotation and the forward's
 * outputs and writes dL/d(raw) from dL/d(activated). */
int gsr_activations_forward(int64_t N, const float *scaling, const float *opacity, const float *rotation,
                            float *scales, float *opacities, float *rotations, void *stream);
int gsr_activations_backward(int64_t N, const float *rotation, const float *scales, const float *opacities,
                             const float *rotations, const float *dL_dscales, const float *dL_dopacities,
                             const float *dL_drotations, float *dL_dscaling, float *dL_dopacity, float *dL_drotation,
                             void *stream);

/* SparseGaussianAdam.step(visibility, N) of the upstream rasterizer package (diff_gaussian_rasterization, taken by
 * the reference's third_party GaussianModel with optimizer_type "sparse_adam": gaussian_model.py:26,194-196).  Each
 * group's n elements are N Gaussians of n / N elements; only the Gaussians with visible[g] != 0 are updated, as
 * m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, p += -lr m / (sqrt(v) + eps) -- no bias correction, `step` is
 * ignored.  visible: N bytes on the device (a torch bool tensor). */
int gsr_sparse_adam_step(const gsr_adam_group *groups, int num_groups, const uint8_t *visible, int64_t N,
                         double beta1, double beta2, double eps, void *stream);

/* densify_and_prune of gs_lightning/modules/gaussian_model.py:184-287 with the optimizer-state re-indexing of
 * gs_lightning_module.py:213-235, in two calls:
 *   gsr_densify_classify  classifies every row (prune / keep / clone / split) and builds the row maps;
 *                         counts[0..2] (device) = rows kept, rows cloned, rows split.  The caller reads the
 *                         counts back, allocates outputs of N_new = kept + cloned + split rows and draws
 *                         z ~ N(0, 1) of shape (split, 3);
 *   gsr_densify_apply     scatters every field (parameters, Adam moments, statistics) into the new arrays.
 * Thresholds are absolute (the reference's *_threshold * spatial_scale already applied). */
typedef struct gsr_densify_args {
    int64_t N;
    const float *opacity;       /* (N) raw (pre-sigmoid) */
    const float *scaling;       /* (N,3) raw (log) */
    const float *max_radii2D;   /* (N) */
    const float *xyz_grad_accum, *xyz_grad_count;  /* (N) */
    float opacity_threshold;    /* prune unless sigmoid(opacity) > threshold */
    float screensize_threshold; /* with apply_screensize: prune unless max_radii2D < threshold */
    float size_threshold;       /* with apply_size: prune unless max(exp(scaling)) < threshold */
    float grad_threshold;       /* clone/split if accum / count >= threshold */
    float clone_size_threshold; /* clone if max(exp(scaling)) < threshold, split otherwise */
    int apply_screensize, apply_size;
} gsr_densify_args;
size_t gsr_densify_workspace_bytes(int64_t N);
/* preserve_idx (N int64): the first counts[0] entries are the kept row indices (the reference's return value). */
int gsr_densify_classify(const gsr_densify_args *args, void *workspace, int32_t *counts, int64_t *preserve_idx,
                         void *stream);

/* The same row maps from a caller's keep mask (N bytes on the device, non-zero = keep) -- pruning by any criterion,
 * e.g. the contribution statistics above: no clones, no splits (counts[1] = counts[2] = 0).  The workspace is then
 * scattered through gsr_densify_apply like gsr_densify_classify's (z may be NULL). */
int gsr_densify_classify_keep(int64_t N, const uint8_t *keep_mask, void *workspace, int32_t *counts,
                              int64_t *preserve_idx, void *stream);

enum { GSR_FIELD_PLAIN = 0, GSR_FIELD_XYZ = 1, GSR_FIELD_SCALING = 2, GSR_FIELD_STAT = 3 };
typedef struct gsr_densify_field {
    const float *src; /* (N, width) */
    float *dst;       /* (N_new, width) */
    const float *src_exp_avg, *src_exp_avg_sq; /* NULL when the parameter has no optimizer state */
    float *dst_exp_avg, *dst_exp_avg_sq;
    int width;
    int kind; /* XYZ: split rows move by R(q)(z*exp(scaling)); SCALING: log(exp(s)/1.6); STAT: zero on copies */
} gsr_densify_field;
/* rotation (N,4) raw quaternions (w,x,y,z), scaling (N,3) raw, z (split,3): the rows the split moves */
int gsr_densify_apply(int64_t N, const void *workspace, const float *rotation, const float *scaling, const float *z,
                      const gsr_densify_field *fields, int num_fields, void *stream);

/* 3DGS-MCMC densification (Kheradmand et al., NeurIPS 2024; gsplat's MCMCStrategy) on the raw parameters the
 * optimizer steps: opacity (N) or (N,1) logit, scaling (N,3) log, rotation (N,4) unnormalised (w,x,y,z), 16-B aligned.
 * Only functions are added: GSR_ABI_VERSION and every struct stay as they are.  All three return GSR_ERR_ARG before any
 * device work on a NULL required pointer, a negative count, or a min_opacity outside (0, 1), and launch nothing (GSR_OK)
 * when there is no row to work on.
 *
 * gsr_mcmc_noise: xyz[g] += Sigma_g (z[g] * gate_g * scale) in place, Sigma = R(q) diag(exp(scaling)^2) R(q)^T with
 *   q = rotation / max(|rotation|, 1e-12), gate = 1 / (1 + exp(-100 ((1 - sigmoid(opacity)) - 0.995))); z (N,3) are the
 *   caller's standard normal draws, scale the caller's xyz learning rate times its noise learning rate. */
int gsr_mcmc_noise(int64_t N, float *xyz, const float *opacity, const float *scaling, const float *rotation,
                   const float *z, float scale, void *stream);

/* gsr_mcmc_relocation: the values alone, for callers with their own layout.  For j in [0, n): i = src_idx[j] (j itself
 *   when src_idx is NULL, then n <= N), r = clamp(ratio[j], 1, 51), o = sigmoid(opacity[i]), s = exp(scaling[i]):
 *     o' = 1 - (1 - o)^(1/r),  c = o / sum_{k<r} C(r,k+1) (-1)^k o'^(k+1) / sqrt(k+1)
 *     new_opacity[j] = logit(clamp(o', min_opacity, 1 - 2^-23)),  new_scaling[j] = log(c s)
 *   ratio[j] is 1 + the number of times row src_idx[j] occurs in src_idx.  activated != 0: opacity and scaling hold
 *   sigmoid / exp values already and the outputs are o' (not clamped) and c s (gsplat's compute_relocation).  o' is
 *   formed in fp32 as -expm1f(log1pf(-o) / r); the alternating sum is accumulated in fp64.  A src_idx[j] outside [0, N)
 *   is skipped (its outputs are not written). */
int gsr_mcmc_relocation(int64_t N, const float *opacity, const float *scaling, int activated, const int64_t *src_idx,
                        const int32_t *ratio, int64_t n, float min_opacity, float *new_opacity, float *new_scaling,
                        void *stream);

/* gsr_mcmc_apply: relocation or growth of every field (gsr_densify_field; kind GSR_FIELD_OPACITY, width 1, and kind
 *   GSR_FIELD_SCALING, width 3, must both be among them) in two launches: the values above from the old parameters into
 *   `values` (n * 4 floats of device scratch), then one launch that moves the rows.  occurrences (N int32): how often
 *   each row occurs in src_idx (an integer histogram such as torch.bincount); the ratio of source i is 1 + occurrences[i].
 *     dst_idx != NULL, relocate, in place on each field's dst (N, width) (src is ignored): every distinct source row
 *       gets its new opacity and scaling, row dst_idx[j] becomes a copy of the updated row src_idx[j] in every
 *       parameter, dst_exp_avg / dst_exp_avg_sq are zeroed at the source rows and kept elsewhere, STAT fields are not
 *       touched.  No row may be both a source and a destination, and no destination may repeat.
 *     dst_idx == NULL, add, from src (N, width) into dst (N + n, width): rows [0, N) are copied with the sources
 *       updated, row N + j is a copy of the updated source j; moments of rows [0, N) are copied, moments and STAT fields
 *       of the new rows are zero.
 *   Duplicate sources store identical bits, so the result is deterministic; no atomics.  A src_idx[j] or dst_idx[j]
 *   outside [0, N) is skipped (add: that new row is zero-filled).  GSR_ERR_ARG also on a field of width <= 0, a field
 *   without dst (add: without src), more than 16 fields, or a missing opacity / scaling field. */
enum { GSR_FIELD_OPACITY = 4 };
int gsr_mcmc_apply(int64_t N, int64_t n, const int64_t *src_idx, const int64_t *dst_idx, const int32_t *occurrences,
                   float min_opacity, float *values, const gsr_densify_field *fields, int num_fields, void *stream);

/* The 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024).  Only functions are added: GSR_ABI_VERSION and every
 * struct stay as they are.  All three return GSR_ERR_ARG before any device work on a NULL pointer or a negative count
 * (the first also on V < 1 or a near_plane that is not finite), and launch nothing (GSR_OK) at P == 0 / N == 0.
 *
 * gsr_mipfilter_rate: per Gaussian i over the V cameras of `cameras`, a (V,16) fp32 device table, 64-B aligned, row k =
 *     [ V_k[0..3][2] | V_k[0..3][0] | V_k[0..3][1] | fx_k, limx_k, limy_k, 0 ]
 *   with V_k the row-vector view matrix (p_view = [p, 1] V_k), fx_k = W_k / (2 tanfovx_k), limx_k = (1 + 2 margin)
 *   tanfovx_k and limy_k likewise: the view-space z = p . row[0..2] + row[3], x from row[4..7], y from row[8..11].
 *   Camera k sees i when z > near_plane, |x| <= limx_k z and |y| <= limy_k z.  seen[i] = the number of cameras that see
 *   i, rate[i] = the maximum of fx_k / z over them (0 when none does), zmin[i] = the minimum z (+inf when none does).
 *   means3D (P,3); rate, zmin (P) fp32 and seen (P) int32 are written whole.  No atomics; two calls give the same bits.
 *
 * gsr_activations_filter3d_forward / _backward: the parameter activations (gsr_activations_forward) with the filter
 *   folded in.  s = exp(scaling), o = sigmoid(opacity), f = filter_3D[i] >= 0 (N):
 *     scales = sqrt(s^2 + f^2),  opacities = o prod_k (s_k / scales_k),  rotations = rotation / max(|rotation|, 1e-12),
 *   so opacities prod scales = o prod s (the Gaussian's integral).  Where f == 0 the outputs are
 *   gsr_activations_forward's bit for bit.  The backward takes the raw parameters and the filter again (not the
 *   forward's outputs) and writes dL/d(raw) from dL/d(activated); filter_3D takes no gradient.  Shapes and alignment as
 *   for gsr_activations_forward. */
int gsr_mipfilter_rate(int64_t P, const float *means3D, int V, const float *cameras, float near_plane, float *rate,
                       float *zmin, int32_t *seen, void *stream);
int gsr_activations_filter3d_forward(int64_t N, const float *scaling, const float *opacity, const float *rotation,
                                     const float *filter_3D, float *scales, float *opacities, float *rotations,
                                     void *stream);
int gsr_activations_filter3d_backward(int64_t N, const float *scaling, const float *opacity, const float *rotation,
                                      const float *filter_3D, const float *dL_dscales, const float *dL_dopacities,
                                      const float *dL_drotations, float *dL_dscaling, float *dL_dopacity,
                                      float *dL_drotation, void *stream);

/* Normal consistency (2DGS, Huang et al., SIGGRAPH 2024): the normals rendered from the Gaussians against the normals
 * of the rendered depth surface.  Only functions are added: GSR_ABI_VERSION and every struct stay as they are.  All five
 * return GSR_ERR_ARG before any device work on a NULL required pointer, a negative P, H <= 0 or W <= 0, H * W above
 * 2^31 - 1, or a tanfov that is not finite and positive.  Conventions are the rasterizer's: row vectors (p_view =
 * [p, 1] viewmatrix), quaternions (w,x,y,z), pixel (x, y) looks along r(x, y) = ((x + 0.5 - W/2) / fx,
 * (y + 0.5 - H/2) / fy, 1) with fx = W / (2 tanfovx), fy = H / (2 tanfovy) (a centred principal point).
 *
 * gsr_geomfeat_forward: out (P,4), the feature block to render with gsr_features_ext.  Per Gaussian i, k = the index of
 *   the smallest of scales[i] (activated; the first on a tie), n_w = column k of R(q / max(|q|, 1e-12)) with R as the
 *   covariance is built from rotations[i], n_v = n_w viewmatrix[:3,:3], z = p_view.z, n_v negated where
 *   n_v . p_view[:3] > 0 (it faces the camera): out[i] = (n_v, z).  means3D, scales (P,3); rotations, out (P,4), 16-B
 *   aligned; viewmatrix (4,4) on the device.  One launch, no atomics; nothing is launched (GSR_OK) at P == 0.
 * gsr_geomfeat_backward: dL_dmeans3D (P,3) (through z only) and dL_drotations (P,4) (through n_v and the
 *   normalisation) from dL_dout (P,4) and the forward's inputs; k and the flip are recomputed (piecewise constant, so
 *   scales take no gradient, and neither does viewmatrix here).  Both outputs are written whole.
 *
 * gsr_normal_consistency_forward: D (1,H,W) the rendered sum of w z (feature channel 3), A (1,H,W) the rendered alpha,
 *   N (3,H,W) the rendered normals (feature channels 0-2, not normalised).  d = D / A where A > 0, else 0;
 *   Pt(x, y) = d r(x, y);  c = (Pt(x, y+1) - Pt(x, y-1)) x (Pt(x+1, y) - Pt(x-1, y));  n_d = c / |c|, and 0 where
 *   |c| = 0 and on the one-pixel border (2DGS's depth_to_normal: a fronto-parallel surface has n_d = (0, 0, -1));
 *   E = 1 - A (N . n_d), exactly 1 where n_d = 0.  E (1,H,W) is written whole, and n_d (3,H,W) too unless it is NULL.
 * gsr_depth_to_normal: n_d alone, the same bits.
 * gsr_normal_consistency_backward: dD, dA (1,H,W) and dN (3,H,W) from dE (1,H,W) with the factor A of E held constant
 *   (2DGS detaches it): dN = -dE A n_d, and D and A take their gradient through d only; where |c| = 0 the normal's
 *   gradient is zero.  A gather: every pixel sums, in a fixed order, what it contributes to the normals of its four
 *   neighbours, whose cross products are recomputed from D and A; nothing is saved by the forward.  No atomics, every
 *   output element is written exactly once (zeros included), two calls give the same bits. */
int gsr_geomfeat_forward(int64_t P, const float *means3D, const float *scales, const float *rotations,
                         const float *viewmatrix, float *out, void *stream);
int gsr_geomfeat_backward(int64_t P, const float *means3D, const float *scales, const float *rotations,
                          const float *viewmatrix, const float *dL_dout, float *dL_dmeans3D, float *dL_drotations,
                          void *stream);
int gsr_normal_consistency_forward(int H, int W, float tanfovx, float tanfovy, const float *D, const float *A,
                                   const float *N, float *E, float *n_d, void *stream);
int gsr_depth_to_normal(int H, int W, float tanfovx, float tanfovy, const float *D, const float *A, float *n_d,
                        void *stream);
int gsr_normal_consistency_backward(int H, int W, float tanfovx, float tanfovy, const float *D, const float *A,
                                    const float *N, const float *dE, float *dD, float *dA, float *dN, void *stream);
/* The same three on the blended surface d = (1 - depth_ratio) D / A + depth_ratio M where A > 0, else 0: M (1,H,W) the
 * median depth map (gsr_median_ext.out_median_depth), depth_ratio 2DGS's (1: the median surface of its bounded scenes,
 * 0: the expected depth), finite (GSR_ERR_ARG otherwise, and on a NULL M).  The backward hands (1 - depth_ratio) of the
 * surface's gradient to D and A through D / A and depth_ratio of it to dM (1,H,W), written whole (0 where A == 0).  Still
 * one launch each way, a gather, no atomics.  The functions above are unchanged: they never read a median. */
int gsr_normal_consistency_forward_surface(int H, int W, float tanfovx, float tanfovy, const float *D, const float *A,
                                           const float *N, const float *M, float depth_ratio, float *E, float *n_d,
                                           void *stream);
int gsr_depth_to_normal_surface(int H, int W, float tanfovx, float tanfovy, const float *D, const float *A,
                                const float *M, float depth_ratio, float *n_d, void *stream);
int gsr_normal_consistency_backward_surface(int H, int W, float tanfovx, float tanfovy, const float *D, const float *A,
                                            const float *N, const float *M, float depth_ratio, const float *dE,
                                            float *dD, float *dA, float *dN, float *dM, void *stream);

/* PLY vertex records <-> parameter fields (the 3DGS checkpoint of gaussian_model.py:112-171 and
 * third_party/.../gaussian_model.py:239-314).  `records` are n fixed-size records of record_bytes each, on the
 * device; `columns` (host array, destination order: field after field, column after column) give each
 * column's byte offset in the record and its PLY type; fields are row-major (n, widths[f]) fp32 device
 * arrays.  unpack converts any scalar PLY type to fp32; pack writes float32 and zero-fills record bytes no
 * column covers (the normals of save_ply).  big_endian selects binary_big_endian records. */
enum { GSR_PLY_FLOAT32 = 0, GSR_PLY_FLOAT64 = 1, GSR_PLY_UINT8 = 2, GSR_PLY_INT8 = 3, GSR_PLY_UINT16 = 4,
       GSR_PLY_INT16 = 5, GSR_PLY_UINT32 = 6, GSR_PLY_INT32 = 7 };
typedef struct gsr_ply_column {
    int32_t offset;
    int32_t type;
} gsr_ply_column;
int gsr_ply_unpack(const uint8_t *records, int64_t n, int record_bytes, int big_endian, const gsr_ply_column *columns,
                   int num_columns, float *const *fields, const int *widths, int num_fields, void *stream);
int gsr_ply_pack(uint8_t *records, int64_t n, int record_bytes, int big_endian, const gsr_ply_column *columns,
                 int num_columns, const float *const *fields, const int *widths, int num_fields, void *stream);

/* Mean squared distance of every point to its 3 nearest other points -- distCUDA2 of
 * gs_lightning/utils/math.py:9-14 (scipy KDTree query k=4, self dropped), used for the scale initialisation
 * of gaussian_model.py:84-91.  Exact (Morton-ordered octree search); points (n,3) fp32, out (n) fp32. */
size_t gsr_knn_workspace_bytes(int64_t n);
int gsr_knn_mean_dist2(int64_t n, const float *points, float *out, void *workspace, void *stream);

/* Buffer sizes the forward will request (host-only arithmetic; for planning and tests). */
size_t gsr_geom_buffer_bytes(int P);
size_t gsr_binning_buffer_bytes(int64_t R, int W, int H);
size_t gsr_image_buffer_bytes(int W, int H);
size_t gsr_bwd_scratch_bytes(int64_t R, int64_t num_big);
size_t gsr_bwd_scratch_bytes_abs(int64_t R, int64_t num_big); /* with gsr_absgrad_ext.dL_dmeans2D_abs */
/* with gsr_features_ext.dL_dout_features: gsr_bwd_scratch_bytes + align256(max(R,1) * B * 4) + align256(max(num_big,1) *
 * B * 4), B = 8 for C <= 8 and 16 above (one channel block's rows; 0 for C outside 1..64) */
size_t gsr_bwd_scratch_bytes_features(int64_t R, int64_t num_big, int C);

/* Byte offsets of the internal arrays inside the three forward buffers (host arithmetic only).  Used by
 * the parity tests to compare the integer binning state (sorted instance list, tile ranges,
 * per-pixel contributor counts) bit for bit against the oracle. */
typedef struct gsr_state_layout {
    /* in: sizeof(gsr_state_layout) as the caller was built (a caller built against an older header passes its
     * smaller size and gets only the fields it knows); out: the size the library filled (from GSR_ABI_VERSION 2
     * on, fields are only ever appended).  0 is taken as the library's own size.  Version-1 callers (before this
     * field existed) are NOT compatible: see gsr_abi_version(). */
    size_t struct_size;
    size_t geom_rec_a, geom_rec_b, geom_rec_c; /* float4, float4, float2 of Gaussian 0's record; Gaussian i's at
                                                  + i * geom_rec_stride */
    size_t geom_tiles, geom_order, geom_inst_off, geom_inst_start, geom_clamped; /* u32, u32, u32, u32, u8 */
    size_t geom_depth_key;    /* u32 float bits of each Gaussian's view depth (0xffffffff: not rendered) */
    size_t geom_expand_rec;   /* uint4 {kept-tile mask lo, hi, rmin.x | rmin.y << 16, rect width} (mask 0 = all) */
    size_t bin_point_list, bin_inv, bin_keys_sorted;                  /* u32 per instance (bin_inv: sorted position of
                                                                         each instance the composite loaded, else
                                                                         0xffffffff: the backward's row markers) */
    size_t bin_sorted_u, bin_inst_gid;                                /* u32 per instance */
    size_t img_final_T, img_n_contrib, img_ranges, img_tile_last;     /* f32/u32 per pixel, uint2/u32 per tile */
    size_t img_tile_loaded;                                           /* u32 per tile */
    size_t geom_rec_stride;                                           /* bytes per render record (48) */
    size_t bin_bk_keys;       /* u64 per instance: the bucket binning's keys (depth bits << 32 | u) grouped by tile */
} gsr_state_layout;
void gsr_state_layout_query(int P, int64_t R, int W, int H, gsr_state_layout *out);

/* Per-stage device timing (hipEvents on the launch stream).  When enabled, every forward/backward
 * records an event pair around each stage; gsr_stage_times() returns the accumulated milliseconds
 * and call counts since the last reset. */
void gsr_set_profiling(int enable);
int gsr_num_stages(void);
const char *gsr_stage_name(int stage);
int gsr_stage_times(double *total_ms, int64_t *calls, int max_stages);
void gsr_reset_stage_times(void);

/* Internal tuning knobs for A/B measurements (e.g. "bucket"; the list is gsr_tuning_name).  GSR_OK, or GSR_ERR_ARG
 * with gsr_last_error() naming the knob when the library has none of that name (the read-only "stat_*" names
 * included): nothing is stored then. */
int gsr_set_tuning(const char *name, int value);
/* gsr_set_tuning(name, GSR_TUNING_UNSET) forgets the knob: its built-in default applies again. */
#define GSR_TUNING_UNSET (-2147483647 - 1)
/* A knob's value (default_value if not set, or unknown).  The forward's read-only statistics are read here too, under
 * "stat_*" names ("stat_depth_passes": the radix passes of the last depth sort, 0 on the bucket path). */
int gsr_get_tuning(const char *name, int default_value);
/* The knobs: their number, and knob i's name and built-in default ("" and 0 outside [0, gsr_num_tunings())). */
int gsr_num_tunings(void);
const char *gsr_tuning_name(int i);
int gsr_tuning_default(int i);

/* Diagnostics: with the "stamp" knob set, the composite kernels record one (start, end, HW_ID, XCC_ID)
 * uint32 quadruple per launch slot (start/end on the 100 MHz real-time clock).  which = 0: render_fwd,
 * 1: render_bwd, 2: radix-sort pass blocks (start, ranked, looked back, end), 3: radix histogram blocks.  Copies up to max_slots quadruples to host memory; returns the count or < 0. */
int gsr_debug_wave_stamps(int which, uint32_t *host_dst, int max_slots);

const char *gsr_last_error(void);
const char *gsr_build_info(void);

/* Stream-ordered hand-off between two streams without events (the multi-view exchange's chunk hand-offs between the
 * compute stream and the collective stream): gsr_stream_signal writes `value` to the 4-B device word `flag` once the
 * stream's earlier work is done (hipStreamWriteValue32); gsr_stream_wait holds the stream's later work until
 * *flag >= value (hipStreamWaitValue32).  gsr_stream_values_supported() is 0 where the device lacks stream wait
 * values (the caller then uses events). */
int gsr_stream_values_supported(void);
int gsr_stream_signal(void *stream, uint32_t *flag, uint32_t value);
int gsr_stream_wait(void *stream, uint32_t *flag, uint32_t value);

/* ABI version of this header.  2: gsr_state_layout gained struct_size at offset 0 and lost img_tile_sorted /
 * img_tile_lastkey (a one-time break: a caller built against a version-1 header reads shifted offsets, so it must
 * check gsr_abi_version() == GSR_ABI_VERSION before using the layout).  From version 2 on, fields of the versioned
 * structs are only appended, and callers built against this header or a later one interoperate.  3: gsr_backward_args,
 * which carries no size field, gained dL_dviewmatrix / dL_dprojmatrix / dL_dcampos at its end (a version-2 caller's
 * struct ends before them, so the library would read past it). */
#define GSR_ABI_VERSION 3
int gsr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GSRAST_H */
