// gsr_features.hip -- per-Gaussian feature channels (gsr_features_ext): features (P,C) composited with the colour
// render's weights w_i(pix) = alpha_i T_i into out_features (C,H,W), and their backward.
//
// Kernels of their own beside render_fwd_v6_kernel / render_bwd_v5_kernel (both at their register budgets), so a call
// without features launches exactly what it launched before.  The two walks read only what the colour forward recorded
// (ReplaySrc, and final_T) and are built from the replay pieces of gsr_replay.h -- tile prologue, pixel setup, batch
// head, and the pair's alpha and pass decision in the composite's staged-record arithmetic (under the "guard" knob its
// guarded decision) -- so the decisions and the weights are those of the colour forward.  Theirs here: the feature
// rows in LDS, the accumulators, the wave reduction, the zero fill of the feature rows and the stores.
//
// Channel blocks: a launch carries FB = 8 (C <= 8) or 16 channels of the C; the walk is repeated per block.  The
// forward's blocks are independent (grid.y); the backward's run one launch after the other, because each ADDS its
// geometry terms into the instance's 40-B gradient row: only the projection g = sum_c f_ic dL/dF_c(pix) of a
// Gaussian's channels onto the pixel's upstream gradient enters dL/dalpha, the scalar "behind" accumulator follows
// D <- D + alpha (g - D) from 0 (no background term), and both are linear in dL/dF, so a block's six moment sums are
// formed with its own D and added.  One wave owns a tile's rows: a plain read-add-store, no atomics.
#include "gsr_replay.h"

namespace gsr {

int feat_block(int C) { return C <= 8 ? 8 : 16; }

// The batch's feature rows, channels [c0, c0 + FB) (zero past C), into LDS: 4-B loads only -- a row of (P,C) with odd C
// is not 16-B aligned.
template <int FB>
__device__ __forceinline__ void feat_load_rows(const float *__restrict__ features, int C, int c0, int cnt, int lane,
                                               const uint32_t *s_gid, float (*s_f)[FB]) {
    for (int e = lane; e < cnt * FB; e += 64) {
        const int j = e / FB, c = e % FB;
        s_f[j][c] = c0 + c < C ? features[(size_t)s_gid[j] * C + (c0 + c)] : 0.f;
    }
}
// One staged row back into registers (16-B LDS reads)
template <int FB>
__device__ __forceinline__ void feat_row(const float *row, float (&f)[FB]) {
#pragma unroll
    for (int c = 0; c < FB; c += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(row + c);
        f[c] = v.x, f[c + 1] = v.y, f[c + 2] = v.z, f[c + 3] = v.w;
    }
}

// ------------------------------------------------------------------------------------------------
// Feature forward (replay): one wave per (tile, channel block), 4 pixels per lane as the composite.  Walks
// point_list[ranges[tile]] up to each pixel's n_contrib; T restarts from 1 and follows the forward's T (1 - alpha),
// the weight is its alpha T and the sum its fmaf(value, weight, sum) in the same order, so with the same values the
// image has the colour image's bits.
// ------------------------------------------------------------------------------------------------
template <int FB, bool GUARD = false>
__global__ __launch_bounds__(64) void feat_fwd_kernel(FeatFwdParams p) {
    __shared__ FwdRec s_rec[REPLAY_BATCH];
    __shared__ uint32_t s_gid[REPLAY_BATCH];
    __shared__ __attribute__((aligned(16))) float s_f[REPLAY_BATCH][FB];
    const int lane = threadIdx.x, c0 = (int)blockIdx.y * FB;
    const ReplayTile t = replay_tile(p.src, (int)blockIdx.x, lane);
    ReplayPixel q[PIX_PER_LANE];
    float T[PIX_PER_LANE], F[PIX_PER_LANE][FB];
#pragma unroll
    for (int k = 0; k < PIX_PER_LANE; k++) {
        q[k] = replay_pixel(p.src, t, k);
        T[k] = 1.0f;
#pragma unroll
        for (int c = 0; c < FB; c++) F[k][c] = 0.f;
    }
    for (uint32_t b0 = 0; b0 < t.tl; b0 += REPLAY_BATCH) {
        const int cnt = (int)min((uint32_t)REPLAY_BATCH, t.tl - b0);
        ReplayBatch bt = replay_batch(p.src, t, t.r0 + b0, +1, cnt, lane, s_rec, s_gid);
        feat_load_rows<FB>(p.features, p.C, c0, cnt, lane, s_gid, s_f);
        wave_lds_sync();
        while (bt.un) {  // the instances that reach a strip, front to back
            const int j = (int)__builtin_ctzll(bt.un);
            bt.un &= ~(1ull << j);
            const ReplayInst in = replay_inst(s_rec, s_gid, j, t.pfx);
            float f[FB];
            feat_row<FB>(s_f[j], f);
#pragma unroll
            for (int k = 0; k < PIX_PER_LANE; k++) {
                if (!((bt.sk[k] >> j) & 1u)) continue;  // wave-uniform
                const ReplayPair pr = replay_pair<GUARD>(p.src, in, b0 + (uint32_t)j, q[k], t.pfx);
                if (pr.pass) {
                    const float wgt = pr.alpha * T[k];
#pragma unroll
                    for (int c = 0; c < FB; c++) F[k][c] = fmaf(f[c], wgt, F[k][c]);
                    T[k] = T[k] * (1 - pr.alpha);
                }
            }
        }
        wave_lds_sync();  // the next batch overwrites the staged records and rows
    }
    const size_t HW = (size_t)p.src.W * p.src.H;
#pragma unroll
    for (int k = 0; k < PIX_PER_LANE; k++) {
        const ReplayPixel e = replay_pixel(p.src, t, k);  // again: its index is not kept over the walk
#pragma unroll
        for (int c = 0; c < FB; c++)
            if (e.inside && c0 + c < p.C) p.out[(size_t)(c0 + c) * HW + e.pid] = F[k][c];
    }
}

void launch_feat_fwd(hipStream_t s, const FeatFwdParams &p) {
    if (p.src.num_tiles <= 0 || p.C <= 0) return;
    const int fb = feat_block(p.C);
    const dim3 grid((uint32_t)p.src.num_tiles, (uint32_t)div_up((uint32_t)p.C, (uint32_t)fb));
    if (fb == 8) replay_launch(s, grid, p, feat_fwd_kernel<8, false>, feat_fwd_kernel<8, true>);
    else replay_launch(s, grid, p, feat_fwd_kernel<16, false>, feat_fwd_kernel<16, true>);
}

// ------------------------------------------------------------------------------------------------
// Feature compositing backward: one wave per tile, one channel block per launch (launched after render_bwd and before
// big_reduce).  The reverse walk of render_bwd: T recovered by T / (1 - alpha) from final_T, one scalar D per pixel from
// 0.  Per contributing (pixel, instance): g = sum_c f_ic dL/dF_c, d = g - D, D <- D + alpha d, q = G d T, and the lane
// accumulates q, q dy, q dy^2 and the block's FB feature weights w dL/dF_c.  Per instance the wave reduces the six
// moments (q, q dx, q dy, q dx^2, q dx dy, q dy^2) and the FB weights together (wave_reduce_store).  After a batch, lane
// j converts instance j's moments to the row's dmean2D / dconic / dopacity form (render_bwd's conversion) and adds
// them to rows[sorted_u[s]][0..5] -- the four weight floats of the row stay -- and the wave stores the FB feature
// weights to frows[sorted_u[s]], the block's scratch rows by expansion index.  live[gid] = 1 for every Gaussian whose
// row or feature row it makes non-zero: preprocess_bwd and the gathers skip the others.
// ------------------------------------------------------------------------------------------------
template <int FB, bool GUARD = false>
__global__ __launch_bounds__(64) void feat_bwd_kernel(FeatBwdParams p) {
    constexpr int NV = FB + 6 <= 16 ? 16 : 32;
    __shared__ FwdRec s_rec[REPLAY_BATCH];
    __shared__ uint32_t s_gid[REPLAY_BATCH];
    __shared__ uint32_t s_row[REPLAY_BATCH];
    __shared__ __attribute__((aligned(16))) float s_f[REPLAY_BATCH][FB];
    __shared__ __attribute__((aligned(16))) float s_red[REPLAY_BATCH][NV];
    const int lane = threadIdx.x, c0 = p.c0;
    const ReplayTile t = replay_tile(p.src, (int)blockIdx.x, lane);
    // the instances the forward loaded but no pixel reached: zero feature rows (render_bwd zeroed their 40-B rows)
    for (uint32_t e = (uint32_t)lane; e < (t.loaded > t.tl ? t.loaded - t.tl : 0u) * FB; e += 64)
        p.frows[(size_t)p.src.sorted_u[t.r0 + t.tl + e / FB] * FB + e % FB] = 0.f;
    if (t.tl == 0) return;

    const size_t HW = (size_t)p.src.W * p.src.H;
    ReplayPixel q[PIX_PER_LANE];
    float T[PIX_PER_LANE], D[PIX_PER_LANE], dF[PIX_PER_LANE][FB];
#pragma unroll
    for (int k = 0; k < PIX_PER_LANE; k++) {
        q[k] = replay_pixel(p.src, t, k);
        T[k] = q[k].inside ? p.final_T[q[k].pid] : 0.f;
        D[k] = 0.f;
#pragma unroll
        for (int c = 0; c < FB; c++)
            dF[k][c] = (q[k].inside && c0 + c < p.C) ? p.dL_dF[(size_t)(c0 + c) * HW + q[k].pid] : 0.f;
    }
    const float hW = 0.5f * p.src.W, hH = 0.5f * p.src.H;

    for (int bend = (int)t.tl; bend > 0; bend -= REPLAY_BATCH) {
        const int cnt = min(REPLAY_BATCH, bend);
        const ReplayBatch bt = replay_batch(p.src, t, t.r0 + (uint32_t)(bend - 1), -1, cnt, lane, s_rec, s_gid);
        if (lane < cnt) s_row[lane] = bt.row;
        feat_load_rows<FB>(p.features, p.C, c0, cnt, lane, s_gid, s_f);
        wave_lds_sync();
        for (int j = 0; j < cnt; j++) {
            bool any = false;
            float m[NV];
#pragma unroll
            for (int v = 0; v < NV; v++) m[v] = 0.f;
            if ((bt.un >> j) & 1ull) {  // wave-uniform: the instance reaches a strip
                const ReplayInst in = replay_inst(s_rec, s_gid, j, t.pfx);
                float f[FB];
                feat_row<FB>(s_f[j], f);
                float Q0 = 0.f, Q1 = 0.f, Q2 = 0.f;
#pragma unroll
                for (int k = 0; k < PIX_PER_LANE; k++) {
                    if (!((bt.sk[k] >> j) & 1u)) continue;  // wave-uniform
                    const ReplayPair pr = replay_pair<GUARD>(p.src, in, (uint32_t)(bend - 1 - j), q[k], t.pfx);
                    if (pr.pass) {
                        any = true;
                        T[k] = T[k] * fast_rcp(1.f - pr.alpha);
                        const float wgt = pr.alpha * T[k];
                        float g = 0.f;
#pragma unroll
                        for (int c = 0; c < FB; c++) {
                            g = fmaf(f[c], dF[k][c], g);
                            m[6 + c] = fmaf(wgt, dF[k][c], m[6 + c]);
                        }
                        const float d = g - D[k];
                        D[k] = fmaf(pr.alpha, d, D[k]);
                        const float q = pr.G * (d * T[k]);
                        const float qdy = q * pr.dy;
                        Q0 += q;
                        Q1 += qdy;
                        Q2 = fmaf(qdy, pr.dy, Q2);
                    }
                }
                // the six moments in gradient-row order (S, Sx, Sy, Sxx, Sxy, Syy): dx is the lane's own
                m[0] = Q0;
                m[1] = Q0 * in.dx;
                m[2] = Q1;
                m[3] = m[1] * in.dx;
                m[4] = Q1 * in.dx;
                m[5] = Q2;
            }
            if (__ballot(any)) wave_reduce_store<NV>(m, s_red[j], lane);
            else if (lane < NV) s_red[j][lane] = 0.f;
        }
        wave_lds_sync();
        bool nz = false;
        if (lane < cnt) {
            const float *u = s_red[lane];
            const float S = u[0], Sx = u[1], Sy = u[2], Sxx = u[3], Sxy = u[4], Syy = u[5];
            const float o = bt.raw_b.y, ca = bt.raw_a.z, cb = bt.raw_a.w, cc = bt.raw_b.x;  // the raw opacity and conic
            float add[6];
            // the fused product spelled out: the compiler's pick followed the registers' layout.  The other a*b + c*d
            // forms of the walks (power2_at, the moment sums) are its choice still: replay_path_bits.json's scenes check
            add[0] = -o * hW * fmaf(cb, Sy, ca * Sx);
            add[1] = -o * hH * fmaf(cb, Sx, cc * Sy);
            add[2] = -0.5f * o * Sxx;
            add[3] = -0.5f * o * Sxy;
            add[4] = -0.5f * o * Syy;
            add[5] = S;
            float2 *row = reinterpret_cast<float2 *>(p.rows + (size_t)s_row[lane] * GRAD_ROW);
#pragma unroll
            for (int h = 0; h < 3; h++) {
                nz = nz || add[2 * h] != 0.f || add[2 * h + 1] != 0.f;
                const float2 r = row[h];
                row[h] = make_float2(r.x + add[2 * h], r.y + add[2 * h + 1]);
            }
#pragma unroll
            for (int c = 0; c < FB; c++) nz = nz || u[6 + c] != 0.f;
            if (p.live && nz) p.live[s_gid[lane]] = 1;
        }
        for (int e = lane; e < cnt * FB; e += 64) {
            const int j = e / FB, c = e % FB;
            p.frows[(size_t)s_row[j] * FB + c] = s_red[j][6 + c];
        }
        wave_lds_sync();  // the next batch overwrites the staged records, rows and sums
    }
}

void launch_feat_bwd(hipStream_t s, const FeatBwdParams &p) {
    if (p.src.num_tiles <= 0) return;
    const dim3 grid((uint32_t)p.src.num_tiles);
    if (feat_block(p.C) == 8) replay_launch(s, grid, p, feat_bwd_kernel<8, false>, feat_bwd_kernel<8, true>);
    else replay_launch(s, grid, p, feat_bwd_kernel<16, false>, feat_bwd_kernel<16, true>);
}

// ------------------------------------------------------------------------------------------------
// Gaussians with more than BIG_GAUSSIAN_TILES instances: one workgroup sums the block's feature rows of all their
// instances (256 / FB instance lanes x FB channels, fixed stride order, then the lanes in order) into bigsum[slot],
// which the gather reads instead of walking the rows.  The count comes from the host, or, when only an upper bound is
// known there, from the device word the preprocess left (big_reduce_kernel's PERSIST form).
// ------------------------------------------------------------------------------------------------
template <int FB>
__global__ __launch_bounds__(256) void feat_big_reduce_kernel(FeatGatherParams p) {
    constexpr int KL = 256 / FB;
    __shared__ float s_p[KL][FB];
    const int c = threadIdx.x % FB, kl = threadIdx.x / FB;
    const uint32_t nb = p.nbig_dev ? *p.nbig_dev : p.nbig;
    for (uint32_t bi = blockIdx.x; bi < nb; bi += gridDim.x) {  // workgroup-uniform
        const uint32_t gidx = p.src.big_list[bi];
        const uint32_t start = p.src.inst_start[gidx], cnt = p.src.tiles[gidx];
        float acc = 0.f;
        for (uint32_t k = (uint32_t)kl; k < cnt; k += KL)
            if (p.src.inv[start + k] != INV_NONE) acc += p.frows[(size_t)(start + k) * FB + c];
        s_p[kl][c] = acc;
        __syncthreads();
        if (threadIdx.x < FB) {
            float tot = 0.f;
            for (int q = 0; q < KL; q++) tot += s_p[q][threadIdx.x];
            p.bigsum[(size_t)bi * FB + threadIdx.x] = tot;
        }
        __syncthreads();  // s_p is rewritten by the next big Gaussian
    }
}

// Feature gather: dL_dfeatures[g][c0 .. c0 + FB) = the Gaussian's feature rows summed in instance order, under the
// tests of every gather (gsr_gather.h: a positive radius, the live flag when the composite marked them, inv !=
// INV_NONE per instance); a big Gaussian takes feat_big_reduce_kernel's sum.  One thread per (Gaussian, channel): a Gaussian's FB
// threads read one 32- or 64-B row segment together.  Every element is written (exact zeros for a Gaussian that is
// culled or that no pixel takes); 4-B stores, the output need only be 4-B aligned.
template <int FB>
__global__ __launch_bounds__(256) void feat_gather_kernel(FeatGatherParams p) {
    const int c = threadIdx.x % FB;
    const int64_t g = (int64_t)blockIdx.x * (256 / FB) + threadIdx.x / FB;
    if (g >= p.P || p.c0 + c >= p.C) return;
    float acc = 0.f;
    if (gather_wanted(p.src, g, p.src.radii[g])) {
        const uint32_t start = p.src.inst_start[g], cnt = p.src.tiles[g];
        if (cnt > BIG_GAUSSIAN_TILES) {
            acc = p.bigsum[(size_t)p.src.big_slot[g] * FB + c];
        } else {
            // four inv words, then four rows, in flight together (abs_gather_kernel's form); added in instance order
            for (uint32_t k0 = 0; k0 < cnt; k0 += 4) {
                bool use[4];
                inv_use4(p.src, start, k0, cnt, use);
                float rw[4];
#pragma unroll
                for (int j = 0; j < 4; j++) rw[j] = use[j] ? p.frows[(size_t)(start + k0 + j) * FB + c] : 0.f;
#pragma unroll
                for (int j = 0; j < 4; j++) acc += rw[j];
            }
        }
    }
    p.out[(size_t)g * p.C + (p.c0 + c)] = acc;
}

void launch_feat_gather(hipStream_t s, const FeatGatherParams &p) {
    if (p.P <= 0) return;
    const uint32_t nbig_launch = p.nbig_dev ? std::min(p.nbig, 2048u) : p.nbig;
    if (feat_block(p.C) == 8) {
        if (nbig_launch) feat_big_reduce_kernel<8><<<nbig_launch, 256, 0, s>>>(p);
        feat_gather_kernel<8><<<div_up((uint32_t)p.P, 256u / 8u), 256, 0, s>>>(p);
    } else {
        if (nbig_launch) feat_big_reduce_kernel<16><<<nbig_launch, 256, 0, s>>>(p);
        feat_gather_kernel<16><<<div_up((uint32_t)p.P, 256u / 16u), 256, 0, s>>>(p);
    }
}

}  // namespace gsr
