// gsr_contrib.hip -- per-Gaussian contribution statistics (gsr_contributions): over the (Gaussian, pixel) pairs the
// colour forward composited, the number of pairs, the sum and the max of v = [m(pix) *] w_i(pix), w_i = alpha_i T_i.
// What pruning and budgeting methods reduce over views (LightGaussian: the sum, RadSplat: the max, Mini-Splatting /
// Taming-3DGS: the hit count, error-based densification: the sum under a per-pixel error m); no gradient is involved.
//
// Kernels of their own beside the composites and the feature kernels, so a call that does not ask for the statistics
// launches exactly what it launched before.  They only READ what the colour forward recorded (ReplaySrc for the walk,
// GatherSrc's inv for the gather) and write a scratch buffer of this call and the three outputs: a backward on the
// same state afterwards is untouched.
//
// Pixels -> Gaussians without float atomics, as the backward does it: the walk reduces each instance's pairs inside its
// wave (the sum by a fixed DPP tree) into the instance's 16-B row, stored by expansion index, so a Gaussian's rows are
// contiguous; the gather then adds each Gaussian's rows in instance order.  Two calls give the same bits.
#include "gsr_replay.h"

namespace gsr {

// Max over the 64 lanes of the bit patterns of non-negative floats (their order is the integers' order); wave-uniform.
// Lanes a partial row mask leaves out keep their own value (update_dpp's old operand).
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp_umax(uint32_t v) {
    return max(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
    v = dpp_umax<0xB1>(v);        // quad_perm [1,0,3,2]
    v = dpp_umax<0x4E>(v);        // quad_perm [2,3,0,1]
    v = dpp_umax<0x141>(v);       // row_half_mirror
    v = dpp_umax<0x140>(v);       // row_mirror -> row maxima in every lane
    v = dpp_umax<0x142, 0xa>(v);  // row_bcast:15 into rows 1, 3
    v = dpp_umax<0x143, 0xc>(v);  // row_bcast:31 into rows 2, 3 (lane 63 = all)
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// ------------------------------------------------------------------------------------------------
// The walk: one wave per tile, 4 pixels per lane, front to back over point_list[ranges[tile]] up to tile_last, built
// from the replay pieces of gsr_replay.h (the batches staged in LDS, the pair test: sorted index below n_contrib and
// the composite's alpha decision); T restarts from 1 and follows the forward's T (1 - alpha), so the weights are the
// colour render's own.  A pixel whose weight m is not > 0 is left out of everything (its n_contrib is read as 0).  Per
// instance that a pixel takes: the count from the strips' ballots, the lane's sum over its 4 pixels in strip order and
// then wave_sum's fixed tree, the max as integers; lane j of the batch keeps instance j's three values and stores its
// row once.  Every instance the forward loaded gets a row: [tile_last, tile_loaded) zeros.
// ------------------------------------------------------------------------------------------------
template <bool GUARD>
__global__ __launch_bounds__(64) void contrib_walk_kernel(ContribWalkParams p) {
    __shared__ FwdRec s_rec[REPLAY_BATCH];
    __shared__ uint32_t s_gid[REPLAY_BATCH];
    const int lane = threadIdx.x;
    const ReplayTile t = replay_tile(p.src, (int)blockIdx.x, lane);
    // the instances the forward loaded but no pixel reached
    for (uint32_t e = t.tl + (uint32_t)lane; e < t.loaded; e += 64)
        p.rows[p.src.sorted_u[t.r0 + e]] = make_uint4(0, 0, 0, 0);
    if (t.tl == 0) return;

    ReplayPixel q[PIX_PER_LANE];
    float T[PIX_PER_LANE], mw[PIX_PER_LANE];
#pragma unroll
    for (int k = 0; k < PIX_PER_LANE; k++) {
        q[k] = replay_pixel(p.src, t, k);
        mw[k] = (q[k].inside && p.pixel_weights) ? p.pixel_weights[q[k].pid] : 1.0f;
        // own read under the weight's mask: replay_pixel's, then a select, ran 3 % slower (replay_path_resources.md)
        q[k].lastc = (q[k].inside && mw[k] > 0.0f) ? p.src.n_contrib[q[k].pid] : 0u;
        T[k] = 1.0f;
    }
    for (uint32_t b0 = 0; b0 < t.tl; b0 += REPLAY_BATCH) {
        const int cnt = (int)min((uint32_t)REPLAY_BATCH, t.tl - b0);
        ReplayBatch bt = replay_batch(p.src, t, t.r0 + b0, +1, cnt, lane, s_rec, s_gid);
        uint32_t my_cnt = 0, my_max = 0;  // instance `lane` of the batch
        float my_sum = 0.f;
        while (bt.un) {  // the instances that reach a strip, front to back
            const int j = (int)__builtin_ctzll(bt.un);
            bt.un &= ~(1ull << j);
            const ReplayInst in = replay_inst(s_rec, s_gid, j, t.pfx);
            uint32_t c = 0;  // wave-uniform
            float ls = 0.f, lm = 0.f;
#pragma unroll
            for (int k = 0; k < PIX_PER_LANE; k++) {
                if (!((bt.sk[k] >> j) & 1u)) continue;  // wave-uniform
                const ReplayPair pr = replay_pair<GUARD>(p.src, in, b0 + (uint32_t)j, q[k], t.pfx);
                c += (uint32_t)__popcll(__ballot(pr.pass));
                if (pr.pass) {
                    const float v = mw[k] * (pr.alpha * T[k]);  // m == 1 without an image: the weight's own bits
                    ls += v;
                    lm = fmaxf(lm, v);
                    T[k] = T[k] * (1 - pr.alpha);
                }
            }
            if (c) {  // wave-uniform: every lane takes part in the reductions
                const float s = wave_sum(ls);
                const uint32_t m = wave_umax(__float_as_uint(lm));
                if (lane == j) my_cnt = c, my_sum = s, my_max = m;
            }
        }
        if (lane < cnt) p.rows[bt.row] = make_uint4(my_cnt, __float_as_uint(my_sum), my_max, 0u);
        wave_lds_sync();  // the next batch overwrites the staged records
    }
}

void launch_contrib_walk(hipStream_t s, const ContribWalkParams &p) {
    if (p.src.num_tiles <= 0) return;
    replay_launch(s, dim3((uint32_t)p.src.num_tiles), p, contrib_walk_kernel<false>, contrib_walk_kernel<true>);
}

// ------------------------------------------------------------------------------------------------
// Gaussians with more than BIG_GAUSSIAN_TILES instances: one workgroup reduces the rows of all their instances (256
// lanes in a fixed stride order, then the lanes in order) into bigsum[slot], which the gather reads instead of walking
// the rows (feat_big_reduce_kernel's form).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void contrib_big_reduce_kernel(ContribGatherParams p) {
    __shared__ uint32_t s_c[256], s_m[256];
    __shared__ float s_s[256];
    const uint32_t nb = p.nbig_dev ? *p.nbig_dev : p.nbig;
    for (uint32_t bi = blockIdx.x; bi < nb; bi += gridDim.x) {  // workgroup-uniform
        const uint32_t gidx = p.src.big_list[bi];
        const uint32_t start = p.src.inst_start[gidx], cnt = p.src.tiles[gidx];
        uint32_t c = 0, m = 0;
        float acc = 0.f;
        for (uint32_t k = threadIdx.x; k < cnt; k += 256)
            if (p.src.inv[start + k] != INV_NONE) {
                const uint4 r = p.rows[start + k];
                c += r.x;
                acc += __uint_as_float(r.y);
                m = max(m, r.z);
            }
        s_c[threadIdx.x] = c, s_s[threadIdx.x] = acc, s_m[threadIdx.x] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t tc = 0, tm = 0;
            float tot = 0.f;
            for (int q = 0; q < 256; q++) tc += s_c[q], tot += s_s[q], tm = max(tm, s_m[q]);
            p.bigsum[bi] = make_uint4(tc, __float_as_uint(tot), tm, 0u);
        }
        __syncthreads();  // the partials are rewritten by the next big Gaussian
    }
}

// The gather: one thread per Gaussian over its rows in instance order, by radius and inv only; every element of the
// outputs is written (exact zeros for a Gaussian that is culled or that no pixel takes), or updated under accumulate.
__global__ __launch_bounds__(256) void contrib_gather_kernel(ContribGatherParams p) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= p.P) return;
    uint32_t c = 0, m = 0;
    float acc = 0.f;
    if (p.src.radii[g] > 0) {
        const uint32_t start = p.src.inst_start[g], cnt = p.src.tiles[g];
        if (cnt > BIG_GAUSSIAN_TILES) {
            const uint4 r = p.bigsum[p.src.big_slot[g]];
            c = r.x, acc = __uint_as_float(r.y), m = r.z;
        } else {
            // four inv words, then four rows, in flight together (abs_gather_kernel's form); added in instance order
            for (uint32_t k0 = 0; k0 < cnt; k0 += 4) {
                bool use[4];
                inv_use4(p.src, start, k0, cnt, use);
                uint4 rw[4];
#pragma unroll
                for (int j = 0; j < 4; j++) rw[j] = use[j] ? p.rows[start + k0 + j] : make_uint4(0, 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    c += rw[j].x;
                    acc += __uint_as_float(rw[j].y);
                    m = max(m, rw[j].z);
                }
            }
        }
    }
    const float mx = __uint_as_float(m);
    if (p.accumulate) {
        if (p.count) p.count[g] += (int64_t)c;
        if (p.wsum) p.wsum[g] = p.wsum[g] + acc;
        if (p.wmax) p.wmax[g] = fmaxf(p.wmax[g], mx);
    } else {
        if (p.count) p.count[g] = (int64_t)c;
        if (p.wsum) p.wsum[g] = acc;
        if (p.wmax) p.wmax[g] = mx;
    }
}

void launch_contrib_big_reduce(hipStream_t s, const ContribGatherParams &p) {
    const uint32_t nbig_launch = p.nbig_dev ? std::min(p.nbig, 2048u) : p.nbig;
    if (p.P > 0 && nbig_launch) contrib_big_reduce_kernel<<<nbig_launch, 256, 0, s>>>(p);
}

void launch_contrib_gather(hipStream_t s, const ContribGatherParams &p) {
    if (p.P <= 0) return;
    contrib_gather_kernel<<<div_up((uint32_t)p.P, 256u), 256, 0, s>>>(p);
}

}  // namespace gsr
