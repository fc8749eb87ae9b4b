// gsr_contrib.hip -- per-Gaussian contribution statistics (gsr_contributions): over the (Gaussian, pixel) pairs the
// colour forward composited, the number of pairs, the sum and the max of v = [m(pix) *] w_i(pix), w_i = alpha_i T_i.
// What pruning and budgeting methods reduce over views (LightGaussian: the sum, RadSplat: the max, Mini-Splatting /
// Taming-3DGS: the hit count, error-based densification: the sum under a per-pixel error m); no gradient is involved.
//
// Kernels of their own beside the composites and the feature kernels, so a call that does not ask for the statistics
// launches exactly what it launched before.  They only READ what the colour forward recorded (point_list, ranges,
// n_contrib, tile_last / tile_loaded, sorted_u, inv, the 48-B render records) and write a scratch buffer of this call
// and the three outputs: a backward on the same state afterwards is untouched.
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
// The walk: one wave per tile, 4 pixels per lane, front to back over point_list[ranges[tile]] up to tile_last, the
// records staged in LDS batches as feat_fwd_kernel stages them; T restarts from 1 and follows the forward's
// T (1 - alpha), the pair test is feat_fwd_kernel's (sorted index below n_contrib, the composite's alpha decision), so
// the weights are the colour render's own.  A pixel whose weight m is not > 0 is left out of everything (its
// n_contrib is read as 0).  Per instance that a pixel takes: the count from the strips' ballots, the lane's sum over
// its 4 pixels in strip order and then wave_sum's fixed tree, the max as integers; lane j of the batch keeps instance
// j's three values and stores its row once.  Every instance the forward loaded gets a row: [tile_last, tile_loaded)
// zeros.
// ------------------------------------------------------------------------------------------------
template <bool GUARD>
__global__ __launch_bounds__(64) void contrib_walk_kernel(ContribWalkParams p) {
    __shared__ FwdRec s_rec[FEAT_BATCH];
    __shared__ uint32_t s_gid[FEAT_BATCH];
    const int lane = threadIdx.x;
    const int tile = blockIdx.x;
    const int tx = tile % p.gx, ty = tile / p.gx;
    const int px = tx * BLOCK_X + (lane & 15);
    const int py0 = ty * BLOCK_Y + (lane >> 4);
    const float pfx = (float)px;
    const float row0 = (float)(ty * BLOCK_Y), col0 = (float)(tx * BLOCK_X);
    const uint32_t r0 = __builtin_amdgcn_readfirstlane(p.ranges[tile].x);
    const uint32_t tl = __builtin_amdgcn_readfirstlane(p.tile_last[tile]);
    const uint32_t loaded = __builtin_amdgcn_readfirstlane(p.tile_loaded[tile]);
    // the instances the forward loaded but no pixel reached
    for (uint32_t e = tl + (uint32_t)lane; e < loaded; e += 64) p.rows[p.sorted_u[r0 + e]] = make_uint4(0, 0, 0, 0);
    if (tl == 0) return;

    float T[PIX_PER_LANE], prow[PIX_PER_LANE], mw[PIX_PER_LANE];
    uint32_t lastc[PIX_PER_LANE];
#pragma unroll
    for (int k = 0; k < PIX_PER_LANE; k++) {
        const int py = py0 + 4 * k;
        const bool inside = px < p.W && py < p.H;
        const size_t pid = inside ? (size_t)py * p.W + px : 0;
        mw[k] = (inside && p.pixel_weights) ? p.pixel_weights[pid] : 1.0f;
        lastc[k] = (inside && mw[k] > 0.0f) ? p.n_contrib[pid] : 0u;
        T[k] = 1.0f;
        prow[k] = (float)py;
    }
    for (uint32_t b0 = 0; b0 < tl; b0 += FEAT_BATCH) {
        const int cnt = (int)min((uint32_t)FEAT_BATCH, tl - b0);
        float4 ra, rb;
        const uint32_t s_me = r0 + b0 + (uint32_t)lane;
        const uint32_t my_m = feat_stage(p.rec, p.point_list, s_me, lane < cnt, lane, s_rec, s_gid, p.strip_exact != 0,
                                         row0, col0, ra, rb);
        const uint32_t my_row = lane < cnt ? p.sorted_u[s_me] : 0u;
        uint64_t sk[PIX_PER_LANE], un = 0;
#pragma unroll
        for (int k = 0; k < PIX_PER_LANE; k++) {
            sk[k] = __ballot((my_m >> k) & 1u);
            un |= sk[k];
        }
        wave_lds_sync();
        uint32_t my_cnt = 0, my_max = 0;  // instance `lane` of the batch
        float my_sum = 0.f;
        while (un) {  // the instances that reach a strip, front to back
            const int j = (int)__builtin_ctzll(un);
            un &= ~(1ull << j);
            const uint32_t idx = b0 + (uint32_t)j;
            const float4 a = s_rec[j].a, b = s_rec[j].b;  // a: x, y, A, B; b: C, o, -, -
            const float dx = a.x - pfx;
            const float P0 = (a.z * dx) * dx, L = a.w * dx;
            uint32_t c = 0;  // wave-uniform
            float ls = 0.f, lm = 0.f;
#pragma unroll
            for (int k = 0; k < PIX_PER_LANE; k++) {
                if (!((sk[k] >> j) & 1u)) continue;  // wave-uniform
                const float power2 = power2_at(b.x, a.y - prow[k], P0, L);
                const float alpha = fminf(0.99f, b.y * __builtin_amdgcn_exp2f(power2));
                const bool pass = idx < lastc[k] && feat_alpha_pass<GUARD>(power2, alpha, p.rec, s_gid[j], pfx, prow[k]);
                c += (uint32_t)__popcll(__ballot(pass));
                if (pass) {
                    const float v = mw[k] * (alpha * T[k]);  // m == 1 without an image: the weight's own bits
                    ls += v;
                    lm = fmaxf(lm, v);
                    T[k] = T[k] * (1 - alpha);
                }
            }
            if (c) {  // wave-uniform: every lane takes part in the reductions
                const float s = wave_sum(ls);
                const uint32_t m = wave_umax(__float_as_uint(lm));
                if (lane == j) my_cnt = c, my_sum = s, my_max = m;
            }
        }
        if (lane < cnt) p.rows[my_row] = make_uint4(my_cnt, __float_as_uint(my_sum), my_max, 0u);
        wave_lds_sync();  // the next batch overwrites the staged records
    }
}

void launch_contrib_walk(hipStream_t s, const ContribWalkParams &p0) {
    if (p0.num_tiles <= 0) return;
    ContribWalkParams p = p0;
    p.strip_exact = tuning("strip_exact", 1);
    const dim3 grid((uint32_t)p.num_tiles), block(64);
    if (tuning("guard", 0)) contrib_walk_kernel<true><<<grid, block, 0, s>>>(p);  // as the colour forward ran
    else contrib_walk_kernel<false><<<grid, block, 0, s>>>(p);
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
