// gsr_kernels.h -- host-side launchers of the HIP kernels (defined in gsr_*.hip).
#pragma once

#include "gsr_common.h"

namespace gsr {

// Diagnostics: per-wave (start, end, HW_ID, XCC_ID) stamps of the composite kernels, one uint4 per launch
// slot, written only when the "stamp" knob is set (buffer 0: render_fwd, 1: render_bwd; 2: the last onesweep
// sort pass, per block (start, ranked, looked back, end); 3: the multi-histogram, per block (start, loop done,
// end, 0)).
uint4 *stamp_buffer(int which);

// ---- scan / sort (gsr_sort.hip) ----
// Exclusive scan of n u32 values (optionally gathered through idx: v[i] = in[idx[i]]).
// out has n+1 entries; out[n] = total.  overflow_flag (device u32) is set if the total exceeds 2^32-1.
// Same result in one launch (decoupled look-back); status (div_up(n + 1, SCAN_TILE) words) and *ticket zeroed.
void launch_exclusive_scan_lookback(hipStream_t s, const uint32_t *in, const uint32_t *idx, uint32_t n, uint32_t *out,
                                    uint64_t *status, uint32_t *ticket, uint32_t *overflow_flag);

// LSD radix sort of n (key, value) pairs on bits [0, nbits).  Keys start in sc.k[0]; values are the
// implicit iota 0..n-1.  After ceil(nbits/8) passes the keys are in sc.k[passes & 1] and the values in
// sc.v[passes & 1].
// LSD radix sort of sc.k[0] (nbits significant bits); values are the iota permutation unless `keyed`, in which
// case sc.v[0] holds the input values.  The result lands in buffer index (passes & 1).
// keys0 (optional): read the first pass's keys from there instead of sc.k[0] (left unmodified).
// gather (optional): the last pass also writes dst[i] = src[sorted value i] for each non-null pair; returns
// whether it did (always, with a gather).
struct SortGather {
    const uint32_t *src = nullptr;
    uint32_t *dst = nullptr;
    const uint4 *src4 = nullptr;
    uint4 *dst4 = nullptr;
};
bool launch_radix_sort(hipStream_t s, SortScratch &sc, uint32_t n, int nbits, bool keyed = false,
                       const uint32_t *keys0 = nullptr, const SortGather *gather = nullptr);
// relative-key depth sort (multi-kernel path, up to 9-bit digits): see gsr_sort.hip
void launch_depth_sort_rel(hipStream_t s, SortScratch &sc, uint32_t n, const uint32_t *keys0, uint32_t kbase,
                           uint32_t kcap, int bits, const SortGather *gather);
// The same sort on 16-bit keys in `passes` digits of digit_bits bits (multi-kernel passes): sc.k[] hold uint16_t keys,
// values as above.  The radix binning's tile sort takes it up to 65536 tiles (tile_sort_plan).
void launch_radix_sort16(hipStream_t s, SortScratch &sc, uint32_t n, int digit_bits, int passes, int bits);  // bits: key bits in use

// ---- forward (gsr_forward.hip) ----
struct PreprocessParams {
    int P, D, M, W, H, gx, gy;
    float tan_fovx, tan_fovy, focal_x, focal_y, scale_modifier;
    int antialiasing;
    int cull;  // exact tile culling (see tile_has_contribution)
    const float *means3D, *opacities, *scales, *rotations, *cov3D_precomp, *colors_precomp, *shs;
    const float *view, *proj, *campos;
    int *radii;
    GeomState g;
    uint32_t *block_sums;  // optional: kept-tile total of every 256-Gaussian block
    // optional: pinned host words; the last preprocess workgroup writes {instance total lo, hi, big count, seq}
    // to host_words[CNT_WORDS .. +4) in one 16-B store (the forward's readback without a copy or an event)
    uint32_t *host_words;
    uint32_t seq;
    int depth_range = 0;  // publish the kept depth keys' range with the instance total (relative depth sort)
    uint4 *stamps = nullptr;  // diagnostics ("stamp" knob): per wave {start, projected, culled, end}, {HW_ID, XCC_ID}
};
void launch_preprocess(hipStream_t s, const PreprocessParams &p);
void launch_zero16(hipStream_t s, void *p, size_t bytes);  // bytes: a multiple of 16, p 16-B aligned

struct ExpandParams {
    uint32_t P, R;
    int gx, gy;
    const uint32_t *order, *inst_off, *tiles;
    const uint4 *exp_rec;
    const uint4 *exp_sorted;  // optional: exp_rec already in depth order (read by rank, no gather)
    uint32_t *exp_owner;      // owner ranks of the block starts (div_up(R, EXP_TILE) + 1 words)
    uint32_t *keys_out, *inst_gid, *inst_start;
    uint16_t *keys16_out;     // optional: 16-bit tile keys (launch_radix_sort16) instead of keys_out
    uint32_t *inv_none;       // optional: inv, set to INV_NONE for every instance here (no separate fill)
};
void launch_expand(hipStream_t s, const ExpandParams &p);

void launch_identify_ranges(hipStream_t s, const uint32_t *keys_sorted, uint32_t R, uint2 *ranges);
void launch_identify_ranges16(hipStream_t s, const uint16_t *keys_sorted, uint32_t R, uint2 *ranges);

// ---- bucket binning (gsr_bin.hip) ----
struct BucketParams {
    uint32_t P, T, nb, gper;  // Gaussians, tiles, walk blocks launched, Gaussians per block
    // walk blocks owning a Gaussian range (nr <= nb).  Blocks nr.. only walk big rects: bk_walk_blocks() is the count
    // the passes use, nr raised to min(nb, big-Gaussian count); the blocks above it exit and their rows are not read
    uint32_t nr;
    uint32_t R;               // instances (scatter; the region partition's grid)
    const uint32_t *nbig;     // big-Gaussian count (device word written by the preprocess)
    int gx;
    const uint32_t *tiles, *depth_key, *big_list;
    const uint32_t *block_sums;  // preprocess block totals (256 Gaussians each)
    uint32_t *inst_start;  // P + 1: written by the count pass (Gaussian-order exclusive scan of tiles)
    const uint4 *exp_rec;
    uint32_t *hist;        // nb x T counts (the count pass writes them; read-only for the column pass)
    uint32_t *hist_pre;    // nb x T column prefixes (column pass), seeding the scatter's bucket slots
    uint32_t *tile_next;   // T: the tiles' starts (column pass), then the region partition's next free slots (atomics)
    uint32_t *tile_start;  // T + 1
    uint2 *ranges;         // T
    uint32_t *long_list;   // 2 x (T + 1): tiles of (SEG_CAP, SEG_BLOCK_CAP] instances, longer tiles
    uint32_t *long_cnt;    // 2 counts (zeroed)
    uint32_t *ticket;      // zeroed: column-pass workgroup ticket
    uint64_t *tile_status; // zeroed: div_up(T, 32) look-back words of the column pass
    uint32_t *err;         // look-back flags (bit 2: a decoupled fallback ran; diagnostic)
    uint32_t lb_patience;  // look-back polls before recomputing an unpublished predecessor
    int lb_force;          // recompute every predecessor (tests the fallback)
    uint32_t *tile_last, *tile_loaded;  // T each: cleared by the column pass for the forward composite
    uint32_t *inv;         // R: reset to INV_NONE beside inst_gid (the forward composite fills it)
    uint32_t *lpt_bcnt;    // 256: cleared by the column pass (the forward's backward-LPT bucket counts)
    unsigned long long *keys;  // R: depth << 32 | u, bucketed by tile
    // region scatter (keys_reg != null; R <= 2^28): the scatter writes each key into its tile's REGION (BK_REGION
    // consecutive tile ids) with the tile's index in the region in bits 28-31 of u (BK_REG_SHIFT), and
    // bk_partition_kernel then moves the keys of each region into their tile buckets (keys), without those bits
    unsigned long long *keys_reg;  // R, or null
    uint32_t *reg_start;           // T / BK_REGION + 2: region starts (tile_start of each region's first tile), column pass
    uint32_t *inst_gid;    // R
    uint32_t *order;       // scatter: an extra workgroup writes the forward LPT order here (or null: none)
    uint32_t *order_xcd;   // and, when set, the per-XCD LPT slot map of the forward composite (xcd_slots(T) words)
    int lpt_shift;
    int xcd_major;         // bucket runs in XCD-major block order (bk_row_block)
};
void launch_bucket_count(hipStream_t s, const BucketParams &p);    // walk + column prefixes + tile ranges
void launch_bucket_scatter(hipStream_t s, const BucketParams &p);

struct SegSortParams {
    uint32_t T;
    const uint2 *ranges;
    const uint32_t *tile_order;  // or null
    unsigned long long *keys;   // R bucketed keys
    unsigned long long *keys2;  // R: chunk-sorted keys of the tiles longer than SEG_BLOCK_CAP
    uint32_t *sorted_u;
    const uint32_t *long_list, *long_cnt;
    uint4 *stamps;  // diagnostics (set by launch): per long-tile slot (start, chunks sorted, end, n), or null
};
void launch_seg_sort(hipStream_t s, const SegSortParams &p);

// Tiles ordered by descending work (range length, or tile_last when use_last) for an LPT launch order.
void launch_tile_order(hipStream_t s, const uint2 *ranges, const uint32_t *tile_last, int use_last, int T,
                       uint32_t *order, uint32_t *scratch = nullptr);  // scratch: ImageState::lpt_hist

struct RenderFwdParams {
    int W, H, gx, gy, num_tiles;
    int xcd;  // tile_order is the per-XCD slot map (order_xcd, XCD_NONE = no tile) and the appends go to the XCD lists
    const uint2 *ranges;
    const uint32_t *tile_order;  // launch slot -> tile (heaviest first), or null for identity
    const uint32_t *sorted_u, *inst_gid;
    uint32_t *point_list, *tile_loaded;
    uint32_t *inv;                        // R: inv[u] = sorted position of every instance the walk loads
    const GRec *rec;
    const float *bg;
    float *out_color, *out_invdepth, *final_T;
    uint32_t *n_contrib, *tile_last;
    uint4 *stamps; // diagnostics (set by launch), or null
    int strip_exact;  // strip skipping mask: 1 strip_mask_exact (column-band extent), 0 strip_mask (set by launch)
    int definite_fast;  // batches of definite conics walk without the exponent-sign test (set by launch)
    // segmented-backward checkpoints (BinningState::ckpt, ImageState::ctot / ck_flag), or null: written every ck_k
    // instances when the launch runs tiles in 4 parts; *ck_flag = ck_k if it did, else 0
    float *ckpt = nullptr, *ctot = nullptr;
    uint32_t *ck_flag = nullptr;
    uint32_t ck_k = 0;
    // backward LPT bucket lists (ImageState::lpt_*), or null: whole-tile waves append their tile; *lpt_valid = 1 if
    // every tile was appended (whole tiles and lists given), else 0
    uint32_t *lpt_bcnt = nullptr, *lpt_blist = nullptr, *lpt_valid = nullptr;
    // exact per-instance strip masks for the backward (BinningState::strip_mask), or null: whole-tile waves record
    // which strips took each loaded instance; *smask_valid = 1 if this launch wrote them, else 0
    uint8_t *strip_mask = nullptr;
    uint32_t *smask_valid = nullptr;
    // gsr_composite_ext: a (3,H,W) background read per pixel in place of bg (bg then points at the image too: it is
    // still read), and the rendered alpha 1 - final_T (H,W); null: the plain epilogue
    const float *bg_image = nullptr;
    float *out_alpha = nullptr;
};
void launch_render_fwd(hipStream_t s, const RenderFwdParams &p);
int render_fwd_parts(int num_tiles);  // row-strip parts per tile launch_render_fwd uses (1: whole tiles)

void launch_mark_visible(hipStream_t s, int P, const float *means3D, const float *view, uint8_t *present);

// ---- backward (gsr_backward.hip) ----
struct RenderBwdParams {
    int W, H, gx, gy, num_tiles;
    const uint2 *ranges;
    const uint32_t *tile_order;  // launch slot -> tile (heaviest first), or null for identity
    const uint32_t *point_list, *n_contrib, *tile_last, *tile_loaded;
    const uint32_t *sorted_u;  // sorted position -> expansion index u: an instance's gradient row is row u
    const GRec *rec;
    const float *bg, *final_T, *dL_dpix, *dL_dinvdepth;
    float *rows;    // R x GRAD_ROW
    uint8_t *live;  // P: set to 1 for the Gaussian of every non-zero row stored (GeomState::live), or null
    uint32_t *live_valid;  // 1 when this composite marked the live flags, 0 when it did not (read by preprocess_bwd)
    uint4 *stamps;  // diagnostics (set by launch), or null
    int strip_exact;  // as RenderFwdParams::strip_exact (set by launch)
    int definite_fast;  // as RenderFwdParams::definite_fast (set by launch)
    uint64_t num_rendered = 0;  // instances (the launch's walk-variant choice)
    // segmented walk (small images): the forward's checkpoints, or null for one wave (or workgroup) per tile
    const float *ckpt = nullptr, *ctot = nullptr;
    const uint32_t *ck_flag = nullptr;
    uint2 *seg_list = nullptr;
    uint32_t *seg_count = nullptr;
    uint32_t ck_k = 0;
    // launch order from the forward's LPT bucket lists when *lpt_valid (else tile_order / identity)
    const uint32_t *lpt_bcnt = nullptr, *lpt_blist = nullptr, *lpt_valid = nullptr;
    // the forward's exact strip masks when *smask_valid (else the conservative cell_mask of the record)
    const uint8_t *strip_mask = nullptr;
    const uint32_t *smask_valid = nullptr;
    // Zero fill of the per-Gaussian backward outputs, spread over the composite's workgroups (bwd_zero_fill): the
    // 16-B aligned interior of each output as segments of one virtual array of zf_total16 uint4, their unaligned
    // head / tail words listed one by one.  preprocess_bwd then stores only the Gaussians with a non-zero gradient.
    static constexpr int ZF_SEGS = 10, ZF_ODD = 60;
    uint32_t zf_nseg = 0, zf_nodd = 0;
    uint64_t zf_total16 = 0;
    uint4 *zf_ptr[ZF_SEGS] = {};
    uint64_t zf_pre16[ZF_SEGS + 1] = {};  // prefix sums of the segments' lengths
    uint32_t *zf_odd[ZF_ODD] = {};
    // gsr_composite_ext: the walk's scalar starts from bg_image(pix) . dL_dpix(pix) (in place of bg, which then points
    // at the image too: it is still read) minus dL_dalpha(pix); null: the plain start
    const float *bg_image = nullptr, *dL_dalpha = nullptr;
    // absolute screen-space sums (gsr_absgrad_ext): R x 8-B rows (sum |m_x|, sum |m_y| of the instance's pixels) by
    // expansion index like `rows`, or null: the kernels without them
    float2 *abs_rows = nullptr;
};
bool launch_render_bwd(hipStream_t s, const RenderBwdParams &p);  // false: nothing to launch (no tile)

// ---- background gradients, empty-scene fill (gsr_background.hip) ----
// dL/dbackground_image = final_T * dL_dpix (3,H,W) and / or dL/dbackground (3) = its sum over the pixels, in one pass
// over final_T (null: 1, no Gaussian) and dL_dpix plus the fixed-order sum of the per-workgroup partials
// (background_partials_bytes(HW) bytes, needed only with dbg).
size_t background_partials_bytes(size_t HW);
void launch_background_grad(hipStream_t s, size_t HW, const float *final_T, const float *dL_dpix, float *dimg,
                            float *dbg, float *partials);
// the forward of a scene without Gaussians: colour = the background (bg_image (3,H,W), else bg (3)), alpha = 0
void launch_background_fill(hipStream_t s, size_t HW, const float *bg, const float *bg_image, float *out_color,
                            float *out_alpha);

// What every per-Gaussian gather of the backward's instance rows reads to decide which rows to add: filled once per
// backward (gsr_api.hip) and embedded in the param structs of the kernels that gather (the decisions themselves:
// gsr_gather.h)
struct GatherSrc {
    const int *radii;
    const uint32_t *tiles, *inst_start, *big_slot, *big_list;
    const uint32_t *inv;  // the forward's inverse permutation: INV_NONE where the composite loaded no instance (no row)
    const uint8_t *live;  // P: 0 = no non-zero row (the gather is skipped: zero sums), or null = gather every Gaussian
    const uint32_t *live_valid;  // the flags are used only when the last composite marked them
};

struct BigReduceParams {
    GatherSrc src;
    const float *rows;
    float *bigsum;  // nbig x GRAD_ROW
    const uint32_t *nbig_dev;  // or null: the launch's nbig is exact; else an upper bound and this the count
    // the instances' abs rows and their per-big-Gaussian sums (nbig x 8 B), or null: the kernels without them
    const float2 *abs_rows = nullptr;
    float2 *bigsum_abs = nullptr;
};
void launch_big_reduce(hipStream_t s, const BigReduceParams &p, uint32_t nbig);

struct PreprocessBwdParams {
    int P, D, M, W, H;
    int g0, g1;  // Gaussians [g0, g1) (the whole [0, P) unless the backward is split into chunks); every output pointer
                 // is indexed by the absolute Gaussian index (the API pre-offsets chunk-relative ones)
    float tan_fovx, tan_fovy, focal_x, focal_y, scale_modifier;
    int antialiasing, has_invdepth;
    int sh_vec16;  // M == 16 and shs / dL_dsh 16-byte aligned: vectorised SH path
    const float *means3D, *opacities, *scales, *rotations, *cov3D_precomp, *shs;
    const float *view, *proj, *campos;
    GatherSrc src;
    const uint8_t *clamped;
    const float *sh_jac;  // 9 x P direction Jacobian of the colour, from the forward (SH degree > 0)
    const float *rows, *bigsum;
    float *dL_dmeans2D, *dL_dcolors, *dL_dopacity, *dL_dmeans3D, *dL_dcov3D, *dL_dsh, *dL_dscales, *dL_drot;
    float *dL_dcolors_sh;  // clamp-masked colour gradient (may be null)
    float *densify_stats;  // (P,2) |dL/dmeans2D[:2]|, radii > 0 (may be null)
    int densify_accumulate;  // densify_stats += instead of =
    int *max_radii2D;        // (P) max(max_radii2D, radii) (may be null)
    float *campos_rows;      // (campos_nrows, 3): campos in row campos_rank, zeros elsewhere (may be null)
    int campos_rank, campos_nrows;
    int prezeroed = 0;       // the outputs were zero-filled (RenderBwdParams::zf_*): store only non-zero gradients
    // camera gradients: camera_partials_bytes(g1 - g0) of per-wave partial sums (null: the kernels without them)
    float *cam_partials = nullptr;
};
void launch_preprocess_bwd(hipStream_t s, const PreprocessBwdParams &p);
// dL_dmeans2D_abs (P,2) over Gaussians [g0, g1): the Gaussian's abs rows summed in the order, and under the same inv /
// big-Gaussian / live tests, as launch_preprocess_bwd sums its 40-B rows.  abs_stats: densify_stats (which the
// per-Gaussian kernel is then not given) is written here, [i][0] from the absolute sums.
struct AbsGatherParams {
    int g0, g1;
    GatherSrc src;
    const float2 *abs_rows, *bigsum_abs;
    float *out;            // (P,2), indexed by the absolute Gaussian index
    float *densify_stats;  // (P,2) or null (abs_stats)
    int densify_accumulate;
    int prezeroed;  // out was zero-filled by the composite: only non-zero rows are stored
};
void launch_abs_gather(hipStream_t s, const AbsGatherParams &p);
// dL/dviewmatrix (16), dL/dprojmatrix (16), dL/dcampos (3) over Gaussians [g0, g1), each fully written or null: the
// fixed-order sum of the partials launch_preprocess_bwd left in p.cam_partials (g1 > g0)
size_t camera_partials_bytes(int64_t n);
void launch_camera_reduce(hipStream_t s, const PreprocessBwdParams &p, float *dview, float *dproj, float *dcampos);

// What every replay of the colour forward reads of the state it recorded: filled once per call (gsr_api.hip) and
// embedded in the param structs of the kernels that replay (the walk's shared pieces: gsr_replay.h)
struct ReplaySrc {
    int W, H, gx, gy, num_tiles;
    const uint2 *ranges;
    const uint32_t *point_list, *n_contrib, *tile_last, *tile_loaded;
    const uint32_t *sorted_u;  // sorted position -> expansion index u: an instance's row is row u
    const GRec *rec;
    int strip_exact = 0;  // as RenderFwdParams::strip_exact (set by launch)
};

// ---- per-Gaussian feature channels (gsr_features.hip) ----
constexpr int FEAT_MAX_C = 64;
int feat_block(int C);  // channels one launch carries: 8 (C <= 8) or 16; the walks repeat per block
// out (C,H,W) = sum_i alpha_i T_i features[i][c], the colour forward's weights replayed from its recorded state
struct FeatFwdParams {
    ReplaySrc src;
    int C;
    const float *features;  // (P,C), 4-B aligned
    float *out;
};
void launch_feat_fwd(hipStream_t s, const FeatFwdParams &p);
// One channel block [c0, c0 + feat_block(C)) of the feature compositing backward, after launch_render_bwd and before
// launch_big_reduce: adds the block's geometry terms into rows[..][0..5] and writes frows (R x feat_block(C) floats by
// expansion index: sum_pix w_i(pix) dL_dF_c(pix))
struct FeatBwdParams {
    ReplaySrc src;
    int C, c0;
    const float *final_T, *features, *dL_dF;  // dL_dF (C,H,W)
    float *rows, *frows;
    uint8_t *live;  // as RenderBwdParams::live, or null
};
void launch_feat_bwd(hipStream_t s, const FeatBwdParams &p);
// out[g][c0 .. c0 + feat_block(C)) of dL_dfeatures (P,C): the Gaussian's frows summed in instance order under
// launch_abs_gather's tests; Gaussians with more than BIG_GAUSSIAN_TILES instances through bigsum (nbig x
// feat_block(C) floats), which the launch fills first
struct FeatGatherParams {
    int P, C, c0;
    GatherSrc src;
    const float *frows;
    float *bigsum;
    uint32_t nbig;             // big Gaussians, or an upper bound with nbig_dev the device's count
    const uint32_t *nbig_dev;  // or null
    float *out;
};
void launch_feat_gather(hipStream_t s, const FeatGatherParams &p);

// ---- depth distortion map (gsr_distortion.hip) ----
enum DistMap : int { DIST_MAP_Z = 0, DIST_MAP_NDC = 1 };  // gsrast.h GSR_DISTORTION_Z / GSR_DISTORTION_NDC
// out (H,W) = sum_i sum_j w_i w_j |t_i - t_j| over the colour forward's pairs, replayed from its recorded state, and
// the per-pixel totals tot_w = sum_i w_i, tot_m = sum_i w_i t_i the backward starts from; all three fully written
struct DistFwdParams {
    ReplaySrc src;
    const uint32_t *depth_key;  // P: float bits of the view depth (GeomState::depth_key)
    int map;
    float k0, nearp;            // DIST_MAP_NDC: t = k0 (1 - nearp / z), k0 = far / (far - near)
    float *out, *tot_w, *tot_m;
};
void launch_dist_fwd(hipStream_t s, const DistFwdParams &p);
// The distortion backward, after launch_render_bwd (and launch_feat_bwd) and before launch_big_reduce: adds its
// geometry terms into rows[..][0..5] and its depth term, as inverse-depth weight, into rows[..][9]
struct DistBwdParams {
    ReplaySrc src;
    const uint32_t *depth_key;
    int map;
    float k0, nearp, dscale;    // dscale = far near / (far - near): z^2 dt/dz of DIST_MAP_NDC
    const float *final_T, *tot_w, *tot_m, *dL_dD;  // (H,W) each
    float *rows;
    uint8_t *live;  // as RenderBwdParams::live, or null
};
void launch_dist_bwd(hipStream_t s, const DistBwdParams &p);

// ---- median depth map (gsr_median.hip) ----
// Per pixel the pair at which the colour forward's transmittance crosses 1/2 (the last contributor whose incoming T
// exceeds 0.5), replayed from its recorded state: the pair's position in the tile's sorted list, its Gaussian id and
// that Gaussian's view depth (-1, -1, 0 where no Gaussian reaches); all three fully written
struct MedianFwdParams {
    ReplaySrc src;
    const uint32_t *depth_key;  // P: float bits of the view depth (GeomState::depth_key)
    float *out_depth;           // (H,W)
    int32_t *out_index, *out_pos;
};
void launch_median_fwd(hipStream_t s, const MedianFwdParams &p);
// The median backward, after launch_render_bwd (and the feature / distortion backward walks) and before
// launch_big_reduce: per selected instance the sum of dL_dmedian over the tile's pixels that selected it, added as
// inverse-depth weight into rows[..][9]
struct MedianBwdParams {
    ReplaySrc src;
    const uint32_t *depth_key;
    const int32_t *pos;         // (H,W): the forward's out_pos
    const float *dL_dmedian;    // (H,W)
    float *rows;
    uint8_t *live;  // as RenderBwdParams::live, or null
};
void launch_median_bwd(hipStream_t s, const MedianBwdParams &p);

// ---- per-Gaussian contribution statistics (gsr_contrib.hip) ----
// The colour forward replayed once more, forward only: per contributing (Gaussian, pixel) pair the value
// v = [m(pix) *] alpha_i T_i; per instance the wave's count, sum and max of v go to the instance's 16-B row
// {count, sum bits, max bits, 0} by expansion index (zeros for a loaded instance no pixel takes).
struct ContribWalkParams {
    ReplaySrc src;
    const float *pixel_weights;  // (H,W) or null: a pixel whose weight is not > 0 is left out
    uint4 *rows;                 // R
};
void launch_contrib_walk(hipStream_t s, const ContribWalkParams &p);
// count / wsum / wmax (P each, any null) from the rows in instance order, by radius and inv only (the live flags belong
// to the backward composite); Gaussians with more than BIG_GAUSSIAN_TILES instances through bigsum (nbig rows), which
// the launch fills first.  accumulate: count +=, wsum = wsum + total, wmax = max(wmax, max).
struct ContribGatherParams {
    int P;
    GatherSrc src;  // live, live_valid: null
    const uint4 *rows;
    uint4 *bigsum;
    uint32_t nbig;             // big Gaussians, or an upper bound with nbig_dev the device's count
    const uint32_t *nbig_dev;  // or null
    int64_t *count;
    float *wsum, *wmax;
    int accumulate;
};
void launch_contrib_big_reduce(hipStream_t s, const ContribGatherParams &p);
void launch_contrib_gather(hipStream_t s, const ContribGatherParams &p);

// ---- multi-view SH gradient (gsr_views.hip) ----
void launch_sh_backward_views(hipStream_t s, int P, int D, int M, int V, int chunk_len, const float *means3D,
                              const float *campos, const float *dcolors_sh, float *dsh);

// One Adam element update (torch's Adam, non-amsgrad, no weight decay), shared by adam_kernel and the fused SH
// Adam so the two give the same bits: the contractions are explicit (the compiler's choice of FMA could differ between
// the kernels otherwise):
//     m = lerp(m, g, 1 - b1);  v = v b2 + (1 - b2) g^2;  p -= step_size * m / (sqrt(v) / sqrt(bc2) + eps)
// Bitwise torch.optim.Adam's step on this device (tests/test_adam.py): mul_(beta2) is a kernel of its own, so v b2
// is rounded before addcmul_ contracts value * (g g) + v; sqrtf is the correctly rounded root (__fsqrt_rn is the
// hardware's approximate one here).
__device__ __forceinline__ void adam_update(float &p, float g, float &m, float &v, float b1c, float b2, float b2c,
                                            float step_size, float bc2_sqrt, float eps) {
#pragma clang fp contract(off)
    m = __fmaf_rn(b1c, __fsub_rn(g, m), m);                // exp_avg.lerp_(grad, 1 - beta1)
    v = __fmaf_rn(b2c, __fmul_rn(g, g), __fmul_rn(v, b2));  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    const float denom = __fadd_rn(__fdiv_rn(sqrtf(v), bc2_sqrt), eps);
    p = __fmaf_rn(-step_size, __fdiv_rn(m, denom), p);     // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// fused Adam of the SH groups on the multi-view expansion (gsr_views.hip; M = 16)
struct AdamShGroup {
    float *param, *exp_avg, *exp_avg_sq;
    float step_size, bc2_sqrt;
    int64_t param_stride;  // floats between the parameter's rows: 3 / 45 (own tensors) or 48 (one (P, 16, 3) tensor)
};
struct AdamShLaunch {
    int P, V, L;
    const float *means3D, *campos, *dc;
    AdamShGroup dc_group, rest_group;
    float one_minus_beta1, beta2, one_minus_beta2, eps;
    int vec4;
    int joint;  // parameter and moments each one 16-B aligned (P, 16, 3) tensor (dc_group's pointers: its base)
};
void launch_adam_sh_views(hipStream_t s, const AdamShLaunch &L, int D);

// ---- fused Adam (gsr_adam.hip) ----
constexpr int ADAM_MAX_GROUPS = 16;
struct AdamGroupDev {
    float *param;
    const float *grad;
    float *exp_avg, *exp_avg_sq;
    int64_t n;
    float step_size, bc2_sqrt;
    int vec4;
    int64_t M;   // sparse step: elements per Gaussian (element e belongs to Gaussian e / M)
    float lr;    // sparse step: the group's learning rate (no bias correction)
};
struct AdamLaunch {
    AdamGroupDev g[ADAM_MAX_GROUPS];
    int64_t slice_start[ADAM_MAX_GROUPS];
    int num_groups;
    float one_minus_beta1, beta2, one_minus_beta2, eps;
    float beta1;                 // sparse step
    const uint8_t *visible;      // sparse step: N bytes, nonzero = the Gaussian was rendered this step
};
int64_t adam_slices(int64_t n);
void launch_adam(hipStream_t s, const AdamLaunch &L, int64_t total_slices);
void launch_sparse_adam(hipStream_t s, const AdamLaunch &L, int64_t total_slices);

// ---- parameter activations (gsr_adam.hip) ----
struct ActivationArgs {
    int64_t N;
    const float *scaling, *opacity, *rotation;        // raw parameters (N,3) (N) (N,4)
    float *scales, *opacities, *rotations;            // forward outputs / backward inputs (activated)
    const float *dL_dscales, *dL_dopacities, *dL_drotations;
    float *dL_dscaling, *dL_dopacity, *dL_drotation;  // backward outputs
};
void launch_activations_forward(hipStream_t s, const ActivationArgs &A);
void launch_activations_backward(hipStream_t s, const ActivationArgs &A);

// ---- densify_and_prune (gsr_densify.hip) ----
struct DensifyParams {
    int64_t N;
    const float *opacity, *scaling, *max_radii2D, *grad_accum, *grad_count;
    float opacity_threshold, screensize_threshold, size_threshold, grad_threshold, clone_size_threshold;
    int apply_screensize, apply_size;
    uint8_t *row_class;      // (N)
    int32_t *block_counts;   // (3 * blocks)
    int32_t *counts;         // (3): kept, cloned, split
    int32_t *dst_map;        // (2N): kept row destination | appended copy destination (-1 = none)
    int32_t *split_rank;     // (N)
    int64_t *preserve_idx;   // (N): first counts[0] entries valid
};
constexpr int DENSIFY_MAX_FIELDS = 16;
struct DensifyFieldDev {
    const float *src, *src_exp_avg, *src_exp_avg_sq;
    float *dst, *dst_exp_avg, *dst_exp_avg_sq;
    int width, kind;
};
struct DensifyApply {
    DensifyFieldDev f[DENSIFY_MAX_FIELDS];
    int64_t block_start[DENSIFY_MAX_FIELDS];
    int num_fields;
    int64_t N;
    const int32_t *dst_map, *split_rank;
    const float *z, *rotation, *scaling;
};
int64_t densify_blocks(int64_t N);
void launch_densify_classify(hipStream_t s, const DensifyParams &p);
// the same maps from a caller's keep mask (N bytes, non-zero = keep): no clones, no splits
void launch_densify_classify_keep(hipStream_t s, const DensifyParams &p, const uint8_t *keep_mask);
void launch_densify_apply(hipStream_t s, const DensifyApply &A, int64_t total_blocks);

// ---- 3DGS-MCMC noise, relocation and growth (gsr_mcmc.hip) ----
struct McmcNoise {
    int64_t N;
    float *xyz;                                       // (N,3), updated in place
    const float *opacity, *scaling, *rotation, *z;    // raw (N) (N,3) (N,4), draws (N,3)
    float scale;
    float gate_c_hi, gate_c_lo;                       // 1 - 0.995 in double, split into two floats
};
void launch_mcmc_noise(hipStream_t s, const McmcNoise &A);

constexpr int MCMC_MAX_RATIO = 51;
struct McmcValues {
    int64_t N, n;
    const float *opacity, *scaling;   // (N) (N,3): raw (logit / log), or activated
    const int64_t *src_idx;           // (n), or null: row j itself
    const int32_t *ratio;             // (n), or null: 1 + occ[src_idx[j]]
    const int32_t *occ;               // (N) occurrences of each row in src_idx (with ratio null)
    float *new_opacity, *new_scaling; // row j at new_opacity + j * op_stride and new_scaling + j * sc_stride
    int op_stride, sc_stride;         // 1 and 3 (packed (n) and (n,3)), or 4 and 4 (one (n,4) temporary)
    int activated;
    float min_opacity;
    double inv_sqrt[MCMC_MAX_RATIO];  // 1 / sqrt(k + 1), formed on the host in double
};
void launch_mcmc_values(hipStream_t s, const McmcValues &A);

struct McmcApply {
    DensifyFieldDev f[DENSIFY_MAX_FIELDS];
    int64_t block_start[DENSIFY_MAX_FIELDS];
    int num_fields;
    int64_t N, n;
    const int64_t *src_idx, *dst_idx;  // dst_idx null: add mode (row N + j)
    const int32_t *occ;                // (N)
    const float *values;               // (n,4): new raw opacity, new raw scaling
};
void launch_mcmc_apply(hipStream_t s, const McmcApply &A, int64_t total_blocks);

// ---- PLY records <-> fields (gsr_ply.hip) ----
constexpr int PLY_MAX_COLS = 128, PLY_MAX_FIELDS = 8;
struct PlyLaunch {
    const uint8_t *records;   // unpack source
    uint8_t *records_out;     // pack destination
    int64_t n;
    int record_bytes, rows_per_block, ncols, nfields, swap;
    float *field[PLY_MAX_FIELDS];
    int width[PLY_MAX_FIELDS];
    int2 cols[PLY_MAX_COLS];  // (byte offset in the record, GSR_PLY_* type), destination order
};
int ply_rows_per_block(int record_bytes);
void launch_ply(hipStream_t s, const PlyLaunch &p, bool pack);

// ---- exact 3-NN mean squared distance (gsr_knn.hip) ----
struct KnnScratch {
    void *base;
    SortScratch sort;
    uint64_t *codes, *scode;
    float4 *spts;
    float *partial, *box;
};
size_t knn_workspace(int64_t n, KnnScratch *k);  // k == nullptr: size only; else carve from k->base
void launch_knn(hipStream_t s, KnnScratch &k, const float *pts, int64_t n, float *out);

// ---- fused SSIM loss (gsr_ssim.hip) ----
size_t ssim_num_partials(int planes, int H, int W);
void launch_ssim_forward(hipStream_t s, int planes, int H, int W, const float *img1, const float *img2, int valid,
                         float *partial, float *d_mu1, float *d_s11, float *d_s12);
void launch_ssim_backward(hipStream_t s, int planes, int H, int W, const float *img1, const float *img2, int valid,
                          const float *dL_dmean, float inv_n, const float *d_mu1, const float *d_s11,
                          const float *d_s12, float *dL_dimg1);

// ---- bilateral-grid colour correction (gsr_bilagrid.hip) ----
constexpr int BG_MAX_BATCH = 8;  // images per slice launch
struct BgShape {
    int L, Gh, Gw, H, W;
};
struct BgBatch {
    int b0;               // first image of the launch
    int g[BG_MAX_BATCH];  // grid of image b0 + blockIdx.z
};
int bilagrid_splits(const BgShape &S);
size_t bilagrid_workspace_bytes(const BgShape &S);
void launch_bilagrid_slice_forward(hipStream_t s, const BgShape &S, int B, const int32_t *idx, const float *grids,
                                   const float *image, float *out);
void launch_bilagrid_slice_backward_image(hipStream_t s, const BgShape &S, int B, const int32_t *idx,
                                          const float *grids, const float *image, const float *dout, float *dimage);
hipError_t launch_bilagrid_slice_backward_grid(hipStream_t s, const BgShape &S, int num, int B, const int32_t *idx,
                                               const float *image, const float *dout, float *dgrids, float *workspace);
size_t bilagrid_tv_num_partials(int num, int L, int Gh, int Gw);
void launch_bilagrid_tv_forward(hipStream_t s, int num, int L, int Gh, int Gw, const float *grids, float *partial);
void launch_bilagrid_tv_backward(hipStream_t s, int num, int L, int Gh, int Gw, const float *grids,
                                 const float *dL_dtv, float *dgrids);

// ---- Mip-Splatting 3D smoothing filter: sampling rates and filtered activations (gsr_mipfilter.hip) ----
struct MipCamera {       // one row of the (V,16) camera table, 64 B
    float zc[4];         // viewmatrix[:, 2]: z = p . zc[:3] + zc[3]
    float xc[4];         // viewmatrix[:, 0]
    float yc[4];         // viewmatrix[:, 1]
    float fx;            // W / (2 tanfovx)
    float limx, limy;    // (1 + 2 margin) tanfovx, (1 + 2 margin) tanfovy
    float pad;
};
static_assert(sizeof(MipCamera) == 64, "the camera table is (V,16) floats");
struct MipRateArgs {
    int64_t P;
    int V;
    float near;
    const float *means3D;       // (P,3)
    const MipCamera *cameras;   // (V)
    float *rate, *zmin;         // (P)
    int32_t *seen;              // (P)
};
void launch_mipfilter_rate(hipStream_t s, const MipRateArgs &A);

struct Filter3DArgs {
    int64_t N;
    const float *scaling, *opacity, *rotation, *filter_3D;  // raw parameters (N,3) (N) (N,4), the filter (N)
    float *scales, *opacities, *rotations;                  // forward outputs
    const float *dL_dscales, *dL_dopacities, *dL_drotations;
    float *dL_dscaling, *dL_dopacity, *dL_drotation;        // backward outputs
};
void launch_activations_filter3d_forward(hipStream_t s, const Filter3DArgs &A);
void launch_activations_filter3d_backward(hipStream_t s, const Filter3DArgs &A);

// ---- normal consistency: geometry features, depth normals and the loss map (gsr_normals.hip) ----
struct GeomfeatArgs {
    int64_t P;
    const float *means3D, *scales, *rotations;  // (P,3) (P,3) activated, (P,4) (w,x,y,z) unnormalised
    const float *viewmatrix;                    // (4,4) row vectors, on the device
    float *out;                                 // forward: (P,4) = (n_v, z)
    const float *dL_dout;                       // backward: (P,4)
    float *dL_dmeans3D, *dL_drotations;         // backward: (P,3) (P,4)
};
void launch_geomfeat_forward(hipStream_t s, const GeomfeatArgs &A);
void launch_geomfeat_backward(hipStream_t s, const GeomfeatArgs &A);

struct NormalArgs {
    int H, W;
    float ifx, ify;           // 2 tanfovx / W, 2 tanfovy / H
    float cx, cy;             // 0.5 - W/2, 0.5 - H/2: the ray of pixel (x, y) is ((x + cx) ifx, (y + cy) ify, 1)
    const float *D, *A, *N;   // (1,H,W) (1,H,W) (3,H,W)
    float *E, *n_d;           // forward: (1,H,W), (3,H,W); either may be null
    const float *dE;          // backward: (1,H,W)
    float *dD, *dA, *dN;      // backward: (1,H,W) (1,H,W) (3,H,W)
    // the blended surface d = (1 - r) D / A + r m (the *_surface entry points; null / 0 otherwise: d = D / A)
    const float *Md;          // (1,H,W) the median depth m, or null
    float ratio;              // r (2DGS's depth_ratio)
    float *dM;                // backward: (1,H,W), with Md
};
void launch_normal_consistency_forward(hipStream_t s, const NormalArgs &A);
void launch_normal_consistency_backward(hipStream_t s, const NormalArgs &A);

}  // namespace gsr
