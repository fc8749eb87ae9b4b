// gsr_median.hip -- the median depth map (gsr_median_ext): per pixel the view depth and the id of the Gaussian at
// which the ray's transmittance crosses 1/2 (2DGS's depth_ratio = 1 surface, its TSDF depth), and its backward.
//
// The fourth user of the replay layer (gsr_replay.h): the forward walks the pairs the colour forward composited, front
// to back, with its alpha (under the "guard" knob its guarded decision), carries T from 1 as the other replays do and
// selects pair i while the transmittance reaching it exceeds 1/2 -- the last contributor with incoming T > 0.5, the
// last contributor at all on a pixel that never becomes half opaque (2DGS's rule).  A selection, not a weighted sum:
// no feature channel can render it.  Unlike the other walks this one stops early: a pixel is finished once T <= 0.5
// (or its contributors end), and the wave leaves the tile's list at the first batch boundary with no unfinished pixel.
//
// The map is piecewise constant in everything but the selected Gaussian's depth, so the backward only sums
// g = dL/dmedian_depth per selected instance and adds it, as inverse-depth weight, to the instance's gradient row (one
// wave owns a tile's rows: a plain read-add-store, no atomics); the row gather, big_reduce and the per-Gaussian pass
// carry it on to means3D and the camera.  No exponential and no scratch of its own: it compares the positions the
// forward saved.
#include "gsr_replay.h"

namespace gsr {

// ------------------------------------------------------------------------------------------------
// Median forward (replay): one wave per tile, 4 pixels per lane as the composite.  Per contributing pair, front to
// back: if T > 0.5 the pair is the median so far; T <- T (1 - alpha).  Writes, for every pixel of the image, the
// selected pair's position in the tile's sorted list (-1: no Gaussian reaches), its Gaussian id (-1) and that
// Gaussian's view depth, the float the preprocess left in depth_key (exactly 0).
// ------------------------------------------------------------------------------------------------
template <bool GUARD>
__global__ __launch_bounds__(64) void median_fwd_kernel(MedianFwdParams p) {
    __shared__ FwdRec s_rec[REPLAY_BATCH];
    __shared__ uint32_t s_gid[REPLAY_BATCH];
    const int lane = threadIdx.x;
    const ReplayTile t = replay_tile(p.src, (int)blockIdx.x, lane);
    ReplayPixel q[PIX_PER_LANE];
    float T[PIX_PER_LANE];
    int sel[PIX_PER_LANE];
#pragma unroll
    for (int k = 0; k < PIX_PER_LANE; k++) {
        q[k] = replay_pixel(p.src, t, k);
        T[k] = 1.0f;
        sel[k] = -1;
    }
    for (uint32_t b0 = 0; b0 < t.tl; b0 += REPLAY_BATCH) {
        const int cnt = (int)min((uint32_t)REPLAY_BATCH, t.tl - b0);
        ReplayBatch bt = replay_batch(p.src, t, t.r0 + b0, +1, cnt, lane, s_rec, s_gid);
        while (bt.un) {  // the instances that reach a strip, front to back
            const int j = (int)__builtin_ctzll(bt.un);
            bt.un &= ~(1ull << j);
            const ReplayInst in = replay_inst(s_rec, s_gid, j, t.pfx);
#pragma unroll
            for (int k = 0; k < PIX_PER_LANE; k++) {
                if (!((bt.sk[k] >> j) & 1u)) continue;  // wave-uniform
                const ReplayPair pr = replay_pair<GUARD>(p.src, in, b0 + (uint32_t)j, q[k], t.pfx);
                if (pr.pass) {
                    if (T[k] > 0.5f) sel[k] = (int)b0 + j;
                    T[k] = T[k] * (1 - pr.alpha);
                }
            }
        }
        wave_lds_sync();  // the next batch overwrites the staged records
        // a pixel is unfinished while it is more than half transparent and its contributors go on past this batch
        bool unfinished = false;
#pragma unroll
        for (int k = 0; k < PIX_PER_LANE; k++)
            unfinished = unfinished || (T[k] > 0.5f && q[k].lastc > b0 + (uint32_t)REPLAY_BATCH);
        if (!__ballot(unfinished)) break;  // wave-uniform
    }
#pragma unroll
    for (int k = 0; k < PIX_PER_LANE; k++) {
        if (!q[k].inside) continue;
        int gid = -1;
        float z = 0.f;
        if (sel[k] >= 0) {
            gid = (int)p.src.point_list[t.r0 + (uint32_t)sel[k]];
            z = __uint_as_float(p.depth_key[gid]);
        }
        p.out_depth[q[k].pid] = z;
        p.out_index[q[k].pid] = gid;
        p.out_pos[q[k].pid] = sel[k];
    }
}

void launch_median_fwd(hipStream_t s, const MedianFwdParams &p) {
    if (p.src.num_tiles <= 0) return;
    replay_launch(s, dim3((uint32_t)p.src.num_tiles), p, median_fwd_kernel<false>, median_fwd_kernel<true>);
}

// ------------------------------------------------------------------------------------------------
// Median backward: one wave per tile, launched after render_bwd (and the feature / distortion backward walks) and
// before big_reduce.  The tile's 256 pixels hold the positions the forward selected; batch after batch of 32
// positions, a lane sorts the g of its pixels whose position lies in the batch into 32 per-lane slots (the others
// stay 0) and the wave reduces the 32 slots in one fixed tree (wave_reduce_store<32>): slot j is the sum of g over
// the pixels that selected position b0 + j, whatever the number of distinct medians in the tile -- a batch no pixel
// selected from is skipped by a ballot.  Lane j then adds the sum as inverse-depth weight to the instance's row, as
// dist_bwd_kernel does for DIST_MAP_Z: rows[sorted_u[r0 + b0 + j]][9] += -sum z^2 (preprocess_bwd: dL/dz -= row[9] /
// z^2), and sets live[gid] where that is non-zero.  Neither alpha nor the guard enters: one kernel.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void median_bwd_kernel(MedianBwdParams p) {
    constexpr int NV = REPLAY_BATCH;
    __shared__ __attribute__((aligned(16))) float s_red[NV];
    const int lane = threadIdx.x;
    const ReplayTile t = replay_tile(p.src, (int)blockIdx.x, lane);
    if (t.tl == 0) return;

    int pos[PIX_PER_LANE];
    float g[PIX_PER_LANE];
#pragma unroll
    for (int k = 0; k < PIX_PER_LANE; k++) {
        const int py = t.py0 + 4 * k;
        const bool inside = t.px < p.src.W && py < p.src.H;
        const size_t pid = inside ? (size_t)py * p.src.W + t.px : 0;
        pos[k] = inside ? p.pos[pid] : -1;
        g[k] = inside ? p.dL_dmedian[pid] : 0.f;
        if (pos[k] >= (int)t.tl) pos[k] = -1;  // (never from this forward: a row past the tile's list is not the wave's)
    }
    for (int b0 = 0; b0 < (int)t.tl; b0 += NV) {
        bool mine = false;
#pragma unroll
        for (int k = 0; k < PIX_PER_LANE; k++) mine = mine || (pos[k] >= b0 && pos[k] < b0 + NV);
        if (!__ballot(mine)) continue;  // wave-uniform: no pixel selected from this batch
        float m[NV];
#pragma unroll
        for (int v = 0; v < NV; v++) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < PIX_PER_LANE; k++) a += pos[k] == b0 + v ? g[k] : 0.f;  // rows top to bottom
            m[v] = a;
        }
        wave_reduce_store<NV>(m, s_red, lane);
        wave_lds_sync();
        if (lane < NV && b0 + lane < (int)t.tl) {
            const float sum = s_red[lane];
            const uint32_t s_me = t.r0 + (uint32_t)(b0 + lane);
            const uint32_t gid = p.src.point_list[s_me];
            const float z = __uint_as_float(p.depth_key[gid]);
            const float zw = -sum * (z * z);  // as inverse-depth weight: preprocess_bwd divides by z^2
            if (zw != 0.f) {
                float2 *row = reinterpret_cast<float2 *>(p.rows + (size_t)p.src.sorted_u[s_me] * GRAD_ROW);
                const float2 r4 = row[4];
                row[4] = make_float2(r4.x, r4.y + zw);
                if (p.live) p.live[gid] = 1;
            }
        }
        wave_lds_sync();  // the next batch overwrites the sums
    }
}

void launch_median_bwd(hipStream_t s, const MedianBwdParams &p) {
    if (p.src.num_tiles <= 0) return;
    median_bwd_kernel<<<dim3((uint32_t)p.src.num_tiles), dim3(64), 0, s>>>(p);
}

}  // namespace gsr
