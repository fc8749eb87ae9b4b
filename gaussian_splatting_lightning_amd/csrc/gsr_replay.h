// gsr_replay.h -- the replay of the colour forward, in one place.  The feature kernels (gsr_features.hip), the
// contribution walk (gsr_contrib.hip) and the distortion walks (gsr_distortion.hip) re-walk what render_fwd_v6_kernel
// recorded (ReplaySrc) and must take exactly the (pixel, instance) pairs it took, with its alpha, or their sums silently
// disagree.  Every helper is force-inlined: what a kernel leaves unused of a helper's result (tile_loaded, the row index,
// lastc) is never loaded, only for that reason.  Also the wave reduction the backward walks share (wave_reduce_store).
#pragma once
#include "gsr_gather.h"

namespace gsr {

constexpr int REPLAY_BATCH = 32;

// One wave per tile, 4 pixels per lane as the composite: the lane's column and first row, the tile's corner, and the
// wave-uniform start of the tile's range, its tile_last and tile_loaded
struct ReplayTile {
    int px, py0;
    float pfx, row0, col0;
    uint32_t r0, tl, loaded;
};
__device__ __forceinline__ ReplayTile replay_tile(const ReplaySrc &s, int tile, int lane) {
    const int tx = tile % s.gx, ty = tile / s.gx;
    ReplayTile t;
    t.px = tx * BLOCK_X + (lane & 15);
    t.py0 = ty * BLOCK_Y + (lane >> 4);
    t.pfx = (float)t.px;
    t.row0 = (float)(ty * BLOCK_Y), t.col0 = (float)(tx * BLOCK_X);
    t.r0 = __builtin_amdgcn_readfirstlane(s.ranges[tile].x);
    t.tl = __builtin_amdgcn_readfirstlane(s.tile_last[tile]);
    t.loaded = __builtin_amdgcn_readfirstlane(s.tile_loaded[tile]);
    return t;
}

// Pixel k of the lane: whether it lies in the image, its index (0 outside), its row, and the sorted index its walk
// ends below (n_contrib; 0 outside, so no pair passes)
struct ReplayPixel {
    bool inside;
    size_t pid;
    float prow;
    uint32_t lastc;
};
__device__ __forceinline__ ReplayPixel replay_pixel(const ReplaySrc &s, const ReplayTile &t, int k) {
    const int py = t.py0 + 4 * k;
    ReplayPixel q;
    q.inside = t.px < s.W && py < s.H;
    q.pid = q.inside ? (size_t)py * s.W + t.px : 0;
    q.prow = (float)py;
    q.lastc = q.inside ? s.n_contrib[q.pid] : 0u;
    return q;
}

// A batch's head: lane j < cnt stages the record and Gaussian id of the instance at sorted position s_me = s0 + j * step
// (step = +1 front to back, -1 back to front) and keeps its raw record; sk[k]: the instances that reach the lanes' strip
// k (cell_mask: conservative, a strip without its bit holds no pixel that passes the alpha test), un their union.
// Ends with the wave's LDS sync.
struct ReplayBatch {
    uint32_t row;  // sorted_u[s_me], the instance's expansion index (loaded here, ahead of the sync, with the record)
    float4 raw_a, raw_b;
    uint64_t sk[PIX_PER_LANE], un;
};
__device__ __forceinline__ ReplayBatch replay_batch(const ReplaySrc &s, const ReplayTile &t, uint32_t s0, int step,
                                                    int cnt, int lane, FwdRec *s_rec, uint32_t *s_gid) {
    ReplayBatch bt{};
    const uint32_t s_me = s0 + (uint32_t)(step * lane);
    uint32_t m = 0;
    if (lane < cnt) {
        const uint32_t gid = s.point_list[s_me];
        bt.row = s.sorted_u[s_me];
        s_gid[lane] = gid;
        bt.raw_a = s.rec[gid].a;
        bt.raw_b = s.rec[gid].b;
        s_rec[lane].a = stage_rec_a(bt.raw_a);
        s_rec[lane].b = stage_rec_b(bt.raw_b);
        m = cell_mask(s.strip_exact != 0, bt.raw_a, bt.raw_b, t.row0, t.col0);
    }
#pragma unroll
    for (int k = 0; k < PIX_PER_LANE; k++) {
        bt.sk[k] = __ballot((m >> k) & 1u);
        bt.un |= bt.sk[k];
    }
    wave_lds_sync();
    return bt;
}

// The composite's alpha decision for one (pixel, instance) pair: power <= 0 and alpha >= 1/255.  GUARD ("guard" knob):
// the forward's guarded decision (gsr_common.h) -- a pair whose alpha lies in the band around 1/255 is re-decided from
// the oracle's own arithmetic on the raw record, exactly as render_fwd_v6_kernel / render_bwd_v5_kernel do, so the
// replay takes the pairs the guarded colour forward took.
template <bool GUARD>
__device__ __forceinline__ bool replay_alpha_pass(float power2, float alpha, const GRec *__restrict__ rec, uint32_t gid,
                                                  float pfx, float pfy) {
    if constexpr (GUARD) {
        if (!(power2 <= 0.0f) || !(alpha >= GUARD_A_LO)) return false;
        if (alpha >= GUARD_A_HI) return true;
        return guard_alpha_pass(rec, gid, pfx, pfy);  // rare
    } else {
        return power2 <= 0.0f && !(alpha < 1.0f / 255.0f);
    }
}

// Staged instance j against the lane's column, once per instance (a: x, y, A, B; b: C, o, -, -) ...
struct ReplayInst {
    float4 a, b;
    float dx, P0, L;
    const uint32_t *gid;  // its Gaussian id in LDS, read only by the guarded decision
};
__device__ __forceinline__ ReplayInst replay_inst(const FwdRec *s_rec, const uint32_t *s_gid, int j, float pfx) {
    ReplayInst in;
    in.a = s_rec[j].a, in.b = s_rec[j].b;
    in.dx = in.a.x - pfx;
    in.P0 = (in.a.z * in.dx) * in.dx, in.L = in.a.w * in.dx;
    in.gid = s_gid + j;
    return in;
}
// ... and against one pixel: G = exp2(power2), alpha = min(0.99, o G), and whether the colour forward took the pair
struct ReplayPair {
    float dy, G, alpha;
    bool pass;
};
template <bool GUARD>
__device__ __forceinline__ ReplayPair replay_pair(const ReplaySrc &s, const ReplayInst &in, uint32_t idx,
                                                  const ReplayPixel &q, float pfx) {
    ReplayPair r;
    r.dy = in.a.y - q.prow;
    const float power2 = power2_at(in.b.x, r.dy, in.P0, in.L);
    r.G = __builtin_amdgcn_exp2f(power2);
    r.alpha = fminf(0.99f, in.b.y * r.G);
    r.pass = idx < q.lastc && replay_alpha_pass<GUARD>(power2, r.alpha, s.rec, *in.gid, pfx, q.prow);
    return r;
}

// ------------------------------------------------------------------------------------------------
// Transposing wave reduction of NV (16 or 32) per-lane values, a plainer relative of wave_reduce_pair_store: each
// level halves the number of values a lane carries by exchanging one half with the partner lane across one lane bit
// (bit 5: v_permlane32_swap, bit 4: v_permlane16_swap, bit 3: row_ror:8, bit 2: row_half_mirror -- whose partner
// 7 - l also flips bits 0 and 1, which the last two levels sum over anyway -- bit 1: quad_perm [2,3,0,1]), and the
// levels left over are plain DPP adds.  Value n's total over the 64 lanes lands in the lanes whose bits spell n
// (n = b5 + 2 b4 + 4 b3 + 8 b2 [+ 16 b1]) and is stored to dst[n].  A fixed tree: bitwise reproducible.  Every lane
// must be active.
// ------------------------------------------------------------------------------------------------
template <int NV>
__device__ __forceinline__ void wave_reduce_store(const float *v, float *__restrict__ dst, int lane) {
    static_assert(NV == 16 || NV == 32, "16 or 32 values");
    float a[NV / 2], b[NV / 4], c[NV / 8], d[NV / 16];
#pragma unroll
    for (int i = 0; i < NV / 2; i++) a[i] = sum_swap32(v[2 * i], v[2 * i + 1]);
#pragma unroll
    for (int i = 0; i < NV / 4; i++) b[i] = sum_swap16(a[2 * i], a[2 * i + 1]);
    const bool h3 = (lane & 8) != 0, h2 = (lane & 4) != 0, h1 = (lane & 2) != 0;
#pragma unroll
    for (int i = 0; i < NV / 8; i++) {
        const float keep = h3 ? b[2 * i + 1] : b[2 * i], send = h3 ? b[2 * i] : b[2 * i + 1];
        c[i] = dpp_xadd<0x128>(keep, send);  // row_ror:8 (= lane ^ 8)
    }
#pragma unroll
    for (int i = 0; i < NV / 16; i++) {
        const float keep = h2 ? c[2 * i + 1] : c[2 * i], send = h2 ? c[2 * i] : c[2 * i + 1];
        d[i] = dpp_xadd<0x141>(keep, send);  // row_half_mirror
    }
    int n = ((lane >> 5) & 1) | ((lane >> 3) & 2) | ((lane >> 1) & 4) | ((lane << 1) & 8);
    float e;
    if constexpr (NV == 32) {
        const float keep = h1 ? d[1] : d[0], send = h1 ? d[0] : d[1];
        e = dpp_xadd<0x4E>(keep, send);  // quad_perm [2,3,0,1]
        n |= (lane << 3) & 16;
    } else {
        e = dpp_add<0x4E>(d[0]);
    }
    e = dpp_add<0xB1>(e);  // quad_perm [1,0,3,2]
    if ((lane & (NV == 32 ? 1 : 3)) == 0) dst[n] = e;
}

// Launch of a replay kernel, one wave per workgroup: strip_exact from its knob, and the kernel's guarded form when the
// colour forward ran with the guard (the same decisions)
template <typename Params>
void replay_launch(hipStream_t s, dim3 grid, const Params &p0, void (*plain)(Params), void (*guarded)(Params)) {
    Params p = p0;
    p.src.strip_exact = tuning(K_strip_exact);
    (tuning(K_guard) ? guarded : plain)<<<grid, dim3(64), 0, s>>>(p);
}

}  // namespace gsr
