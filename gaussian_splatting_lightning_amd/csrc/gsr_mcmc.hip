// gsr_mcmc.hip -- 3DGS-MCMC densification (Kheradmand et al., NeurIPS 2024; MCMCStrategy of gsplat): the per-step
// noise on the means, the relocation values, and one row-move launch for relocation and growth.
//
//   noise       xyz[g] += Sigma (z[g] gate scale),  Sigma = R(q) diag(exp(scaling)^2) R(q)^T,
//               gate = 1 / (1 + exp(-100 ((1 - o) - 0.995))),  o = sigmoid(opacity[g]).  One thread per Gaussian,
//               68 B each (56 read, 12 written), HBM-bound.  Sigma v is formed as R (s^2 o (R^T v)).  The gate's
//               exponent is 100 ((1 - 0.995) - o) with 1 - 0.995 carried as two floats: the literal (1 - o) - 0.995
//               rounds 1 - o to an ulp of one, 6e-6 relative in a gate that matters only where o is near 0.005.
//   values      the new opacity and scale of a Gaussian that is relocated onto / copied r - 1 times:
//               o' = 1 - (1 - o)^(1/r),  c = o / D,  D = sum_{k<r} C(r,k+1) (-1)^k o'^(k+1) / sqrt(k+1)
//               (the paper's double sum through the hockey-stick identity).  o' is -expm1f(log1pf(-o) / r) in fp32.
//               The alternating sum is accumulated in fp64 from that fp32 o': at r = 51 its terms reach 1e4 times the
//               sum, so an fp32 accumulation loses up to 3e-4 of c (measured on the host in numpy) where the fp64 one
//               keeps c within an fp32 ulp; binomials by the exact integer recurrence, 1/sqrt(k+1) from a host table.
//   apply       every field (parameters, Adam moments, statistics) in one launch, after the values were written to a
//               temporary from the old parameters: relocate (in place: destination rows become copies of their updated
//               sources, source moments are zeroed) or add (out of place: rows [0, N) copied, row N + j a copy of
//               updated source j with zero moments and statistics).  Duplicate sources compute and store identical
//               bits; no atomics.  An index outside [0, N) is skipped (add mode: that new row is zero-filled).
#include "gsr_kernels.h"
#include "gsrast.h"

namespace gsr {

__global__ __launch_bounds__(256) void mcmc_noise_kernel(McmcNoise A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.N) return;
    const float o = 1.0f / (1.0f + expf(-A.opacity[i]));
    const float gate = 1.0f / (1.0f + expf(-100.0f * ((A.gate_c_hi - o) + A.gate_c_lo)));
    const float g = gate * A.scale;
    const float v0 = A.z[3 * i] * g, v1 = A.z[3 * i + 1] * g, v2 = A.z[3 * i + 2] * g;
    const float e0 = expf(A.scaling[3 * i]), e1 = expf(A.scaling[3 * i + 1]), e2 = expf(A.scaling[3 * i + 2]);
    const float4 q = *reinterpret_cast<const float4 *>(A.rotation + 4 * i);
    // R(q) of the normalised quaternion (w, x, y, z), as densify_apply_kernel's split_offset builds it
    const float nq = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-12f);
    const float w = q.x / nq, x = q.y / nq, y = q.z / nq, z = q.w / nq;
    const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x;
    const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const float r00 = 1.f - (tyy + tzz), r01 = txy - twz, r02 = txz + twy;
    const float r10 = txy + twz, r11 = 1.f - (txx + tzz), r12 = tyz - twx;
    const float r20 = txz - twy, r21 = tyz + twx, r22 = 1.f - (txx + tyy);
    const float u0 = (r00 * v0 + r10 * v1 + r20 * v2) * (e0 * e0);  // s^2 o (R^T v)
    const float u1 = (r01 * v0 + r11 * v1 + r21 * v2) * (e1 * e1);
    const float u2 = (r02 * v0 + r12 * v1 + r22 * v2) * (e2 * e2);
    A.xyz[3 * i] += r00 * u0 + r01 * u1 + r02 * u2;
    A.xyz[3 * i + 1] += r10 * u0 + r11 * u1 + r12 * u2;
    A.xyz[3 * i + 2] += r20 * u0 + r21 * u1 + r22 * u2;
}

void launch_mcmc_noise(hipStream_t s, const McmcNoise &A) {
    if (A.N > 0) mcmc_noise_kernel<<<(unsigned)((A.N + 255) / 256), 256, 0, s>>>(A);
}

__global__ __launch_bounds__(256) void mcmc_values_kernel(McmcValues A) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= A.n) return;
    const int64_t i = A.src_idx ? A.src_idx[j] : j;
    if (i < 0 || i >= A.N) return;
    int r = A.ratio ? A.ratio[j] : 1 + A.occ[i];
    r = min(max(r, 1), MCMC_MAX_RATIO);
    float o = A.opacity[i], s0 = A.scaling[3 * i], s1 = A.scaling[3 * i + 1], s2 = A.scaling[3 * i + 2];
    float log1mo;  // log(1 - o); from the logit x it is -log(1 + e^x), which keeps the digits 1 - sigmoid(x) drops near one
    if (!A.activated) {
        log1mo = -log1pf(expf(o));
        o = 1.0f / (1.0f + expf(-o));
        s0 = expf(s0); s1 = expf(s1); s2 = expf(s2);
    } else {
        log1mo = log1pf(-o);
    }
    float no = -expm1f(log1mo / (float)r);
    const double x = (double)no;
    double D = 0.0, p = x, binom = (double)r;  // C(r, 1) o'
#pragma unroll 1
    for (int k = 0; k < r; k++) {
        const double t = binom * A.inv_sqrt[k] * p;
        D += (k & 1) ? -t : t;
        p *= x;
        binom = binom * (double)(r - 1 - k) / (double)(k + 2);  // C(r, k + 2)
    }
    const float c = D > 0.0 ? (float)((double)o / D) : 1.0f;  // o = 0 (a logit below -88): the limit of o / D
    s0 *= c; s1 *= c; s2 *= c;
    if (!A.activated) {
        no = fminf(fmaxf(no, A.min_opacity), 1.0f - 1.1920929e-7f);  // 1 - 2^-23
        no = logf(no / (1.0f - no));
        s0 = logf(s0); s1 = logf(s1); s2 = logf(s2);
    }
    A.new_opacity[j * A.op_stride] = no;
    float *ns = A.new_scaling + j * A.sc_stride;
    ns[0] = s0; ns[1] = s1; ns[2] = s2;
}

void launch_mcmc_values(hipStream_t s, const McmcValues &A) {
    if (A.n > 0) mcmc_values_kernel<<<(unsigned)((A.n + 255) / 256), 256, 0, s>>>(A);
}

__global__ __launch_bounds__(256) void mcmc_apply_kernel(McmcApply A) {
    int fi = 0;
#pragma unroll 1
    while (fi + 1 < A.num_fields && (int64_t)blockIdx.x >= A.block_start[fi + 1]) fi++;
    const DensifyFieldDev &F = A.f[fi];
    const int64_t w = F.width;
    int64_t e = ((int64_t)blockIdx.x - A.block_start[fi]) * 256 + threadIdx.x;
    const bool add = A.dst_idx == nullptr;
    const bool valued = F.kind == GSR_FIELD_OPACITY || F.kind == GSR_FIELD_SCALING;
    if (add) {
        const int64_t n_old = A.N * w;
        if (e < n_old) {  // rows [0, N): copied; a source's opacity and scaling come from its append thread
            if (!(valued && A.occ[e / w] > 0)) F.dst[e] = F.src[e];
            if (F.dst_exp_avg) F.dst_exp_avg[e] = F.src_exp_avg[e];
            if (F.dst_exp_avg_sq) F.dst_exp_avg_sq[e] = F.src_exp_avg_sq[e];
            return;
        }
        e -= n_old;
    }
    if (e >= A.n * w) return;
    const int64_t j = e / w;
    const int c = (int)(e - j * w);
    const int64_t i = A.src_idx[j];
    const bool ok = i >= 0 && i < A.N;
    if (add) {
        const int64_t od = (A.N + j) * w + c;
        if (F.dst_exp_avg) F.dst_exp_avg[od] = 0.f;
        if (F.dst_exp_avg_sq) F.dst_exp_avg_sq[od] = 0.f;
        if (!ok || F.kind == GSR_FIELD_STAT) {
            F.dst[od] = 0.f;
            return;
        }
        const float v = valued ? A.values[4 * j + (F.kind == GSR_FIELD_SCALING ? 1 + c : 0)] : F.src[i * w + c];
        F.dst[od] = v;
        if (valued) F.dst[i * w + c] = v;
        return;
    }
    const int64_t d = A.dst_idx[j];
    if (!ok || d < 0 || d >= A.N) return;
    const int64_t oi = i * w + c;
    const float v = valued ? A.values[4 * j + (F.kind == GSR_FIELD_SCALING ? 1 + c : 0)] : F.dst[oi];
    F.dst[d * w + c] = v;
    if (valued) F.dst[oi] = v;
    if (F.dst_exp_avg) F.dst_exp_avg[oi] = 0.f;
    if (F.dst_exp_avg_sq) F.dst_exp_avg_sq[oi] = 0.f;
}

void launch_mcmc_apply(hipStream_t s, const McmcApply &A, int64_t total_blocks) {
    if (total_blocks > 0) mcmc_apply_kernel<<<(unsigned)total_blocks, 256, 0, s>>>(A);
}

}  // namespace gsr
