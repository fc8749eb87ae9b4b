// gsr_distortion.hip -- the depth distortion loss of Mip-NeRF 360 (2DGS's / gsplat's distloss) as a per-pixel map
// (gsr_distortion_ext):  D(pix) = sum_i sum_j w_i w_j |t_i - t_j|  over the pairs the colour forward composited,
// w_i = alpha_i T_i the colour render's own weights and t_i a per-Gaussian depth (view depth z, or 2DGS's bounded
// t = far / (far - near) (1 - near / z)), and its backward.
//
// Kernels of their own beside the composites, the third user of the replay layer (gsr_replay.h): the walks read only
// what the colour forward recorded and take its pairs with its alpha (under the "guard" knob its guarded decision).
// The first whose per-pair coefficient depends on the pixel's running state: a tile's list is sorted by view depth and
// both maps are non-decreasing in z, so t is non-decreasing along a pixel's walk and the double sum is the single pass
//     D = 2 sum_i w_i (t_i A_<i - M_<i),   A_<i = sum_(j<i) w_j,  M_<i = sum_(j<i) w_j t_j.
// The forward carries (T, A, M, D) per pixel and saves the totals A, M; the reverse walk of the backward carries the
// suffix sums A_>i, M_>i and takes the prefix sums as total - suffix - own.  No scratch of its own: the geometry terms
// and the depth term are added into the instance's 40-B gradient row (one wave owns a tile's rows: a plain
// read-add-store, no atomics), so the row gather, big_reduce and the per-Gaussian pass carry them on unchanged.
#include "gsr_replay.h"

namespace gsr {

// The map's per-Gaussian depth from the view depth the preprocess left in depth_key (its float bits): DIST_MAP_Z the
// depth itself, DIST_MAP_NDC k0 (1 - near / z) with k0 = far / (far - near).  Every operation rounded once, the same
// in both walks: non-decreasing in z as computed.
__device__ __forceinline__ float dist_depth(int map, float k0, float nearp, float z) {
    return map == DIST_MAP_NDC ? __fmul_rn(k0, __fsub_rn(1.0f, __fdiv_rn(nearp, z))) : z;
}

// ------------------------------------------------------------------------------------------------
// Distortion forward (replay): one wave per tile, 4 pixels per lane as the composite.  Per contributing pair, front to
// back: D += w (t A - M), A += w, M += w t, T <- T (1 - alpha).  Writes 2 D and the totals A, M of every pixel of the
// image (exact zeros where no Gaussian reaches).
// ------------------------------------------------------------------------------------------------
template <bool GUARD>
__global__ __launch_bounds__(64) void dist_fwd_kernel(DistFwdParams p) {
    __shared__ FwdRec s_rec[REPLAY_BATCH];
    __shared__ uint32_t s_gid[REPLAY_BATCH];
    __shared__ float s_t[REPLAY_BATCH];
    const int lane = threadIdx.x;
    const ReplayTile t = replay_tile(p.src, (int)blockIdx.x, lane);
    ReplayPixel q[PIX_PER_LANE];
    float T[PIX_PER_LANE], A[PIX_PER_LANE], M[PIX_PER_LANE], D[PIX_PER_LANE];
#pragma unroll
    for (int k = 0; k < PIX_PER_LANE; k++) {
        q[k] = replay_pixel(p.src, t, k);
        T[k] = 1.0f;
        A[k] = M[k] = D[k] = 0.f;
    }
    for (uint32_t b0 = 0; b0 < t.tl; b0 += REPLAY_BATCH) {
        const int cnt = (int)min((uint32_t)REPLAY_BATCH, t.tl - b0);
        ReplayBatch bt = replay_batch(p.src, t, t.r0 + b0, +1, cnt, lane, s_rec, s_gid);
        if (lane < cnt) s_t[lane] = dist_depth(p.map, p.k0, p.nearp, __uint_as_float(p.depth_key[s_gid[lane]]));
        wave_lds_sync();
        while (bt.un) {  // the instances that reach a strip, front to back
            const int j = (int)__builtin_ctzll(bt.un);
            bt.un &= ~(1ull << j);
            const ReplayInst in = replay_inst(s_rec, s_gid, j, t.pfx);
            const float tj = s_t[j];
#pragma unroll
            for (int k = 0; k < PIX_PER_LANE; k++) {
                if (!((bt.sk[k] >> j) & 1u)) continue;  // wave-uniform
                const ReplayPair pr = replay_pair<GUARD>(p.src, in, b0 + (uint32_t)j, q[k], t.pfx);
                if (pr.pass) {
                    const float wgt = pr.alpha * T[k];
                    D[k] = fmaf(wgt, fmaf(tj, A[k], -M[k]), D[k]);
                    A[k] += wgt;
                    M[k] = fmaf(wgt, tj, M[k]);
                    T[k] = T[k] * (1 - pr.alpha);
                }
            }
        }
        wave_lds_sync();  // the next batch overwrites the staged records and depths
    }
#pragma unroll
    for (int k = 0; k < PIX_PER_LANE; k++) {
        const ReplayPixel e = replay_pixel(p.src, t, k);  // again: its index is not kept over the walk
        if (e.inside) {
            p.out[e.pid] = 2.0f * D[k];
            p.tot_w[e.pid] = A[k];
            p.tot_m[e.pid] = M[k];
        }
    }
}

void launch_dist_fwd(hipStream_t s, const DistFwdParams &p) {
    if (p.src.num_tiles <= 0) return;
    replay_launch(s, dim3((uint32_t)p.src.num_tiles), p, dist_fwd_kernel<false>, dist_fwd_kernel<true>);
}

// ------------------------------------------------------------------------------------------------
// Distortion backward: one wave per tile, launched after render_bwd (and the feature backward) and before big_reduce.
// The reverse walk of render_bwd: T recovered by T / (1 - alpha) from final_T, the suffix sums As, Ms from 0, the
// prefix sums from the forward's totals (A_< = A_tot - A_> - w: the cancellation is DESIGN.md §5's), and one scalar
// "behind" accumulator R per pixel from 0 (no background term).  Per contributing pair, with g = dL/dD(pix):
//     dA = A_< - A_>,  c = 2 [t dA - M_< + M_>]  (= dD/dw_i),  the depth term  g 2 w dA  (= g dD/dt_i),
//     d = g c - R,  R <- R + alpha d,  q = G d T   -- the feature backward with g c where its projection stands.
// Per instance the wave reduces the six moments (q, q dx, q dy, q dx^2, q dx dy, q dy^2) and the depth term together
// (wave_reduce_store<16>).  After a batch, lane j converts instance j's moments to the row's dmean2D / dconic /
// dopacity form (render_bwd's conversion) and adds them to rows[sorted_u[s]][0..5]; the depth term times dt/dz enters
// dL/dz where the inverse-depth term does, as the equivalent contribution to the row's inverse-depth weight
// rows[..][9] (preprocess_bwd: dL/dz -= row[9] / z^2):  -term z^2 for DIST_MAP_Z, -term far near / (far - near) for
// DIST_MAP_NDC, whose dt/dz is that over z^2.  live[gid] = 1 for every Gaussian whose row it makes non-zero.
// ------------------------------------------------------------------------------------------------
template <bool GUARD>
__global__ __launch_bounds__(64) void dist_bwd_kernel(DistBwdParams p) {
    constexpr int NV = 16;
    __shared__ FwdRec s_rec[REPLAY_BATCH];
    __shared__ uint32_t s_gid[REPLAY_BATCH];
    __shared__ uint32_t s_row[REPLAY_BATCH];
    __shared__ float s_t[REPLAY_BATCH];
    __shared__ __attribute__((aligned(16))) float s_red[REPLAY_BATCH][NV];
    const int lane = threadIdx.x;
    const ReplayTile t = replay_tile(p.src, (int)blockIdx.x, lane);
    if (t.tl == 0) return;

    ReplayPixel q[PIX_PER_LANE];
    float T[PIX_PER_LANE], R[PIX_PER_LANE], As[PIX_PER_LANE], Ms[PIX_PER_LANE];
    float At[PIX_PER_LANE], Mt[PIX_PER_LANE], g2[PIX_PER_LANE];
#pragma unroll
    for (int k = 0; k < PIX_PER_LANE; k++) {
        q[k] = replay_pixel(p.src, t, k);
        T[k] = q[k].inside ? p.final_T[q[k].pid] : 0.f;
        R[k] = As[k] = Ms[k] = 0.f;
        At[k] = q[k].inside ? p.tot_w[q[k].pid] : 0.f;
        Mt[k] = q[k].inside ? p.tot_m[q[k].pid] : 0.f;
        g2[k] = q[k].inside ? 2.0f * p.dL_dD[q[k].pid] : 0.f;
    }
    const float hW = 0.5f * p.src.W, hH = 0.5f * p.src.H;

    for (int bend = (int)t.tl; bend > 0; bend -= REPLAY_BATCH) {
        const int cnt = min(REPLAY_BATCH, bend);
        const ReplayBatch bt = replay_batch(p.src, t, t.r0 + (uint32_t)(bend - 1), -1, cnt, lane, s_rec, s_gid);
        float zme = 1.f;
        if (lane < cnt) {
            s_row[lane] = bt.row;
            zme = __uint_as_float(p.depth_key[s_gid[lane]]);
            s_t[lane] = dist_depth(p.map, p.k0, p.nearp, zme);
        }
        wave_lds_sync();
        for (int j = 0; j < cnt; j++) {
            bool any = false;
            float m[NV];
#pragma unroll
            for (int v = 0; v < NV; v++) m[v] = 0.f;
            if ((bt.un >> j) & 1ull) {  // wave-uniform: the instance reaches a strip
                const ReplayInst in = replay_inst(s_rec, s_gid, j, t.pfx);
                const float tj = s_t[j];
                float Q0 = 0.f, Q1 = 0.f, Q2 = 0.f, Z = 0.f;
#pragma unroll
                for (int k = 0; k < PIX_PER_LANE; k++) {
                    if (!((bt.sk[k] >> j) & 1u)) continue;  // wave-uniform
                    const ReplayPair pr = replay_pair<GUARD>(p.src, in, (uint32_t)(bend - 1 - j), q[k], t.pfx);
                    if (pr.pass) {
                        any = true;
                        T[k] = T[k] * fast_rcp(1.f - pr.alpha);
                        const float wgt = pr.alpha * T[k];
                        const float wt = wgt * tj;
                        const float Al = (At[k] - As[k]) - wgt, Ml = (Mt[k] - Ms[k]) - wt;  // the prefix sums
                        const float dA = Al - As[k];
                        const float gc = g2[k] * fmaf(tj, dA, Ms[k] - Ml);
                        Z = fmaf(g2[k] * wgt, dA, Z);
                        As[k] += wgt;
                        Ms[k] += wt;
                        const float d = gc - R[k];
                        R[k] = fmaf(pr.alpha, d, R[k]);
                        const float qq = pr.G * (d * T[k]);
                        const float qdy = qq * pr.dy;
                        Q0 += qq;
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
                m[6] = Z;
            }
            if (__ballot(any)) wave_reduce_store<NV>(m, s_red[j], lane);
            else if (lane < NV) s_red[j][lane] = 0.f;
        }
        wave_lds_sync();
        if (lane < cnt) {
            const float *u = s_red[lane];
            const float S = u[0], Sx = u[1], Sy = u[2], Sxx = u[3], Sxy = u[4], Syy = u[5];
            const float o = bt.raw_b.y, ca = bt.raw_a.z, cb = bt.raw_a.w, cc = bt.raw_b.x;  // the raw opacity and conic
            float add[6];
            add[0] = -o * hW * fmaf(cb, Sy, ca * Sx);
            add[1] = -o * hH * fmaf(cb, Sx, cc * Sy);
            add[2] = -0.5f * o * Sxx;
            add[3] = -0.5f * o * Sxy;
            add[4] = -0.5f * o * Syy;
            add[5] = S;
            // the depth term as inverse-depth weight: preprocess_bwd divides by z^2
            const float zw = -u[6] * (p.map == DIST_MAP_NDC ? p.dscale : zme * zme);
            bool nz = zw != 0.f;
            float2 *row = reinterpret_cast<float2 *>(p.rows + (size_t)s_row[lane] * GRAD_ROW);
#pragma unroll
            for (int h = 0; h < 3; h++) {
                nz = nz || add[2 * h] != 0.f || add[2 * h + 1] != 0.f;
                const float2 r = row[h];
                row[h] = make_float2(r.x + add[2 * h], r.y + add[2 * h + 1]);
            }
            const float2 r4 = row[4];
            row[4] = make_float2(r4.x, r4.y + zw);
            if (p.live && nz) p.live[s_gid[lane]] = 1;
        }
        wave_lds_sync();  // the next batch overwrites the staged records, depths and sums
    }
}

void launch_dist_bwd(hipStream_t s, const DistBwdParams &p) {
    if (p.src.num_tiles <= 0) return;
    replay_launch(s, dim3((uint32_t)p.src.num_tiles), p, dist_bwd_kernel<false>, dist_bwd_kernel<true>);
}

}  // namespace gsr
