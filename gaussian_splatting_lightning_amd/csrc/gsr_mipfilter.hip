// gsr_mipfilter.hip -- the 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024): per-Gaussian sampling rates
// over all training cameras, and the activations with the filter folded in.
//
//   rate        one thread per Gaussian, all V cameras in a loop.  Camera k is row k of a packed (V,16) float table
//               (MipCamera; layout in INTEGRATION.md): the three columns of the row-vector view matrix the test needs,
//               fx, and the two frustum limits (1 + 2 margin) tan.  The row index is the loop counter, the same in every
//               lane, and the table pointer is a kernel argument, so the compiler reads a row with scalar loads (one
//               16-dword load per camera and wave, through the scalar cache) into SGPRs, which the VALU takes as
//               operands directly: no LDS, no barrier, no chunk seam.  Visible: z > near, |x| <= limx z, |y| <= limy z,
//               in multiplied form.  seen = the count, rate = max fx / z, zmin = min z over the visible cameras (0 and
//               +inf when there is none).  12 B read and 12 B written per Gaussian; VALU-bound from a few cameras on.
//               No atomics.
//   activations s = exp(a), o = sigmoid(b), f = filter_3D:  s' = sqrt(s^2 + f^2),  o' = o prod_k (s_k / s'_k),
//               rotations as the plain activations.  The compensation is the product of the three ratios, each of
//               order one; the published sqrt(prod s^2 / prod s'^2) underflows in fp32 from raw scalings near -15.
//               Where f == 0 the plain values are selected, so those rows are activate()'s bit for bit.
//               Forward 68 B per Gaussian (36 read, 32 written).  The backward reads the raw parameters again and
//               recomputes s, s', o and the unit quaternion from them (the forward's expressions, so the same bits)
//               instead of reading the forward's outputs: 100 B per Gaussian (68 read, 32 written), no s'^2 - f^2
//               cancellation, and autograd keeps no activated tensor alive.
//                 dL/da_k = g_s'k s_k (s_k / s'_k) + g_o' o' (f / s'_k)^2,   dL/db = g_o' c o (1 - o).
#include "gsr_kernels.h"
#include "gsrast.h"

namespace gsr {

constexpr float MIP_NORMALIZE_EPS = 1e-12f;  // torch.nn.functional.normalize's eps, as the plain activations

typedef float mip_row_t __attribute__((ext_vector_type(16)));  // a MipCamera as one 64-B aligned vector
static_assert(sizeof(mip_row_t) == sizeof(MipCamera), "one table row");

__global__ __launch_bounds__(256) void mipfilter_rate_kernel(MipRateArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.P) return;
    const float px = A.means3D[3 * i], py = A.means3D[3 * i + 1], pz = A.means3D[3 * i + 2];
    const mip_row_t *__restrict__ cams = reinterpret_cast<const mip_row_t *>(A.cameras);
    const float near = A.near;
    int seen = 0;
    float rate = 0.0f, zmin = __builtin_inff();
    // wave-uniform address: one 16-dword scalar load per camera, taken whole so that fx is there before the branch, and
    // one camera ahead so that its latency runs under this camera's arithmetic
    mip_row_t next = cams[0];
#pragma unroll 2
    for (int k = 0; k < A.V; k++) {
        const mip_row_t c = next;
        next = cams[min(k + 1, A.V - 1)];
        const float z = fmaf(px, c[0], fmaf(py, c[1], fmaf(pz, c[2], c[3])));
        const float x = fmaf(px, c[4], fmaf(py, c[5], fmaf(pz, c[6], c[7])));
        const float y = fmaf(px, c[8], fmaf(py, c[9], fmaf(pz, c[10], c[11])));
        const bool vis = z > near && fabsf(x) <= c[13] * z && fabsf(y) <= c[14] * z;
        if (vis) {  // a wave with no visible lane skips the division
            seen++;
            rate = fmaxf(rate, c[12] / z);
            zmin = fminf(zmin, z);
        }
    }
    A.rate[i] = rate;
    A.zmin[i] = zmin;
    A.seen[i] = seen;
}

void launch_mipfilter_rate(hipStream_t s, const MipRateArgs &A) {
    if (A.P > 0) mipfilter_rate_kernel<<<(unsigned)((A.P + 255) / 256), 256, 0, s>>>(A);
}

__global__ __launch_bounds__(256) void activations_filter3d_forward_kernel(Filter3DArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.N) return;
    const float f = A.filter_3D[i];
    const float o = 1.0f / (1.0f + expf(-A.opacity[i]));
    float c = 1.0f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float s = expf(A.scaling[3 * i + k]);
        const float sf = sqrtf(s * s + f * f);
        c *= s / sf;
        A.scales[3 * i + k] = f == 0.0f ? s : sf;
    }
    A.opacities[i] = f == 0.0f ? o : o * c;
    const float4 q = *reinterpret_cast<const float4 *>(A.rotation + 4 * i);
    const float n = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), MIP_NORMALIZE_EPS);
    *reinterpret_cast<float4 *>(A.rotations + 4 * i) = make_float4(q.x / n, q.y / n, q.z / n, q.w / n);
}

__global__ __launch_bounds__(256) void activations_filter3d_backward_kernel(Filter3DArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.N) return;
    const float f = A.filter_3D[i];
    const float o = 1.0f / (1.0f + expf(-A.opacity[i]));
    const float go = A.dL_dopacities[i];
    float s[3], r[3], t[3], c = 1.0f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        s[k] = expf(A.scaling[3 * i + k]);
        const float sf = sqrtf(s[k] * s[k] + f * f);
        r[k] = s[k] / sf;  // s / s'
        t[k] = f / sf;     // f / s'
        c *= r[k];
    }
    if (f == 0.0f) {  // the plain activations' chain rule
#pragma unroll
        for (int k = 0; k < 3; k++) A.dL_dscaling[3 * i + k] = A.dL_dscales[3 * i + k] * s[k];
        A.dL_dopacity[i] = go * (1.0f - o) * o;
    } else {
        const float w = go * (o * c);  // g_o' o'
#pragma unroll
        for (int k = 0; k < 3; k++)
            A.dL_dscaling[3 * i + k] = A.dL_dscales[3 * i + k] * (s[k] * r[k]) + w * (t[k] * t[k]);
        A.dL_dopacity[i] = go * c * ((1.0f - o) * o);
    }
    const float4 q = *reinterpret_cast<const float4 *>(A.rotation + 4 * i);
    const float4 g = *reinterpret_cast<const float4 *>(A.dL_drotations + 4 * i);
    const float nr = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    float4 d;
    if (nr > MIP_NORMALIZE_EPS) {  // d(q / |q|) = (g - u (u . g)) / |q|
        const float4 u = make_float4(q.x / nr, q.y / nr, q.z / nr, q.w / nr);
        const float ug = u.x * g.x + u.y * g.y + u.z * g.z + u.w * g.w;
        d = make_float4((g.x - u.x * ug) / nr, (g.y - u.y * ug) / nr, (g.z - u.z * ug) / nr, (g.w - u.w * ug) / nr);
    } else {                       // clamped norm: q / eps is linear in q
        d = make_float4(g.x / MIP_NORMALIZE_EPS, g.y / MIP_NORMALIZE_EPS, g.z / MIP_NORMALIZE_EPS,
                        g.w / MIP_NORMALIZE_EPS);
    }
    *reinterpret_cast<float4 *>(A.dL_drotation + 4 * i) = d;
}

void launch_activations_filter3d_forward(hipStream_t s, const Filter3DArgs &A) {
    if (A.N > 0) activations_filter3d_forward_kernel<<<(unsigned)((A.N + 255) / 256), 256, 0, s>>>(A);
}

void launch_activations_filter3d_backward(hipStream_t s, const Filter3DArgs &A) {
    if (A.N > 0) activations_filter3d_backward_kernel<<<(unsigned)((A.N + 255) / 256), 256, 0, s>>>(A);
}

}  // namespace gsr
