// gsr_normals.hip -- normal consistency (2DGS, Huang et al., SIGGRAPH 2024): the per-Gaussian geometry features the
// rasterizer renders as feature channels, and the normals of the rendered depth surface with the loss map.
//
//   geomfeat    one thread per Gaussian, one launch each way, no atomics.  g[i] = (n_v, z): the axis of the smallest
//               scale (first index on a tie) of R(q / |q|), taken to view space by the row-vector view matrix
//               (p_view = [p, 1] V) and turned to face the camera (n_v . p_view <= 0), with the view depth z.  The 16
//               matrix entries are kernel-argument loads at wave-uniform addresses (scalar loads).  Forward 56 B per
//               Gaussian (40 read, 16 written); the backward reads the inputs again, recomputes the axis index and the
//               flip from them (both piecewise constant) and writes dL/dmeans3D (through z only) and dL/drotations
//               (through n_v and the normalisation): 84 B per Gaussian.  scales take no gradient.
//   consistency d = D / A where A > 0, else 0;  Pt(x, y) = d r(x, y),  r = ((x + 0.5 - W/2) / fx, (y + 0.5 - H/2) / fy, 1);
//               c = (Pt(x, y+1) - Pt(x, y-1)) x (Pt(x+1, y) - Pt(x-1, y)),  n_d = c / |c| (0 on the one-pixel border
//               and where |c| = 0),  E = 1 - A (N . n_d).  The forward is one pass, one pixel per thread, the four
//               neighbours through the vector cache: 24 B per pixel (36 with n_d).
//               The backward is a gather.  dd(q), the gradient of d at pixel q, is the sum in a fixed order of what q
//               contributes to the normals of the centres (x, y-1), (x, y+1), (x-1, y), (x+1, y); each centre's cross
//               product is recomputed by the forward's own expression, nothing is saved.  A workgroup owns a 64x16
//               tile: d with a two-pixel halo (68x20) and G = dE A N with a one-pixel halo (3 x 66x18) are staged in
//               LDS (19.7 KB), then every thread walks four rows of the tile, five cross products per pixel (its own
//               for dN).  Every output element is written exactly once, zeros included; no atomics; 44 B per pixel
//               (24 read, 20 written) plus the halo re-reads, which the L2 serves.
#include "gsr_kernels.h"
#include "gsrast.h"

namespace gsr {

constexpr float GEOMFEAT_NORMALIZE_EPS = 1e-12f;  // torch.nn.functional.normalize's eps, as the activations

// Column k of R(u) for the unit quaternion u = (r, x, y, z), R as quat_to_rot builds it.
__device__ __forceinline__ float3 geomfeat_axis(int k, float r, float x, float y, float z) {
    if (k == 0) return make_float3(1.f - 2.f * (y * y + z * z), 2.f * (x * y + r * z), 2.f * (x * z - r * y));
    if (k == 1) return make_float3(2.f * (x * y - r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z + r * x));
    return make_float3(2.f * (x * z + r * y), 2.f * (y * z - r * x), 1.f - 2.f * (x * x + y * y));
}

struct GeomfeatRow {
    int k;         // index of the smallest scale
    float4 u;      // unit quaternion
    float nrm;     // |q|
    float3 nv;     // view-space axis before the flip
    float3 pv;     // view-space mean
    bool flip;
};

__device__ __forceinline__ GeomfeatRow geomfeat_row(const GeomfeatArgs &A, int64_t i) {
    GeomfeatRow g;
    const float s0 = A.scales[3 * i], s1 = A.scales[3 * i + 1], s2 = A.scales[3 * i + 2];
    g.k = 0;
    float sm = s0;
    if (s1 < sm) { g.k = 1; sm = s1; }
    if (s2 < sm) g.k = 2;
    const float4 q = *reinterpret_cast<const float4 *>(A.rotations + 4 * i);
    g.nrm = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    const float n = fmaxf(g.nrm, GEOMFEAT_NORMALIZE_EPS);
    g.u = make_float4(q.x / n, q.y / n, q.z / n, q.w / n);
    const float3 nw = geomfeat_axis(g.k, g.u.x, g.u.y, g.u.z, g.u.w);
    const float *__restrict__ V = A.viewmatrix;  // V[4 * i + j], row vectors
    g.nv = make_float3(nw.x * V[0] + nw.y * V[4] + nw.z * V[8], nw.x * V[1] + nw.y * V[5] + nw.z * V[9],
                       nw.x * V[2] + nw.y * V[6] + nw.z * V[10]);
    const float px = A.means3D[3 * i], py = A.means3D[3 * i + 1], pz = A.means3D[3 * i + 2];
    g.pv = make_float3(px * V[0] + py * V[4] + pz * V[8] + V[12], px * V[1] + py * V[5] + pz * V[9] + V[13],
                       px * V[2] + py * V[6] + pz * V[10] + V[14]);
    g.flip = g.nv.x * g.pv.x + g.nv.y * g.pv.y + g.nv.z * g.pv.z > 0.f;
    return g;
}

__global__ __launch_bounds__(256) void geomfeat_forward_kernel(GeomfeatArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.P) return;
    const GeomfeatRow g = geomfeat_row(A, i);
    const float s = g.flip ? -1.f : 1.f;
    *reinterpret_cast<float4 *>(A.out + 4 * i) = make_float4(s * g.nv.x, s * g.nv.y, s * g.nv.z, g.pv.z);
}

__global__ __launch_bounds__(256) void geomfeat_backward_kernel(GeomfeatArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.P) return;
    const GeomfeatRow g = geomfeat_row(A, i);
    const float4 up = *reinterpret_cast<const float4 *>(A.dL_dout + 4 * i);
    const float *__restrict__ V = A.viewmatrix;
    A.dL_dmeans3D[3 * i] = up.w * V[2];
    A.dL_dmeans3D[3 * i + 1] = up.w * V[6];
    A.dL_dmeans3D[3 * i + 2] = up.w * V[10];
    const float s = g.flip ? -1.f : 1.f;
    const float vx = s * up.x, vy = s * up.y, vz = s * up.z;  // dL/dn_v before the flip
    // dL/dn_w = V[:3,:3] dL/dn_v
    const float g0 = V[0] * vx + V[1] * vy + V[2] * vz;
    const float g1 = V[4] * vx + V[5] * vy + V[6] * vz;
    const float g2 = V[8] * vx + V[9] * vy + V[10] * vz;
    const float r = g.u.x, x = g.u.y, y = g.u.z, z = g.u.w;
    float4 du;  // dL/du, the derivative of geomfeat_axis's column k
    if (g.k == 0)
        du = make_float4(2.f * (z * g1 - y * g2), 2.f * (y * g1 + z * g2), -4.f * y * g0 + 2.f * (x * g1 - r * g2),
                         -4.f * z * g0 + 2.f * (r * g1 + x * g2));
    else if (g.k == 1)
        du = make_float4(2.f * (x * g2 - z * g0), -4.f * x * g1 + 2.f * (y * g0 + r * g2), 2.f * (x * g0 + z * g2),
                         -4.f * z * g1 + 2.f * (y * g2 - r * g0));
    else
        du = make_float4(2.f * (y * g0 - x * g1), -4.f * x * g2 + 2.f * (z * g0 - r * g1),
                         -4.f * y * g2 + 2.f * (r * g0 + z * g1), 2.f * (x * g0 + y * g1));
    float4 d;
    if (g.nrm > GEOMFEAT_NORMALIZE_EPS) {  // d(q / |q|) = (g - u (u . g)) / |q|
        const float ug = r * du.x + x * du.y + y * du.z + z * du.w;
        d = make_float4((du.x - r * ug) / g.nrm, (du.y - x * ug) / g.nrm, (du.z - y * ug) / g.nrm,
                        (du.w - z * ug) / g.nrm);
    } else {                               // clamped norm: q / eps is linear in q
        d = make_float4(du.x / GEOMFEAT_NORMALIZE_EPS, du.y / GEOMFEAT_NORMALIZE_EPS, du.z / GEOMFEAT_NORMALIZE_EPS,
                        du.w / GEOMFEAT_NORMALIZE_EPS);
    }
    *reinterpret_cast<float4 *>(A.dL_drotations + 4 * i) = d;
}

void launch_geomfeat_forward(hipStream_t s, const GeomfeatArgs &A) {
    if (A.P > 0) geomfeat_forward_kernel<<<(unsigned)((A.P + 255) / 256), 256, 0, s>>>(A);
}

void launch_geomfeat_backward(hipStream_t s, const GeomfeatArgs &A) {
    if (A.P > 0) geomfeat_backward_kernel<<<(unsigned)((A.P + 255) / 256), 256, 0, s>>>(A);
}

// ---- depth normals and the consistency map ----

constexpr int NC_TW = 64, NC_TH = 16;                  // the backward's tile
constexpr int NC_DW = NC_TW + 4, NC_DH = NC_TH + 4;    // d with a two-pixel halo
constexpr int NC_GW = NC_TW + 2, NC_GH = NC_TH + 2;    // G with a one-pixel halo
constexpr int NC_ROWS = NC_TH / 4;                     // rows per thread (256 threads as 64 x 4)

__device__ __forceinline__ float nc_rx(const NormalArgs &A, int x) { return ((float)x + A.cx) * A.ifx; }
__device__ __forceinline__ float nc_ry(const NormalArgs &A, int y) { return ((float)y + A.cy) * A.ify; }
__device__ __forceinline__ bool nc_interior(const NormalArgs &A, int x, int y) {
    return x >= 1 && x < A.W - 1 && y >= 1 && y < A.H - 1;
}

__device__ __forceinline__ float3 nc_cross3(float3 a, float3 b) {
    return make_float3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

// The cross product of centre (x, y) from the depths below (y+1), above (y-1), right (x+1) and left (x-1) of it:
// the points first, then their differences, as the definition states them.  Both passes use this one expression.
__device__ __forceinline__ float3 nc_centre(const NormalArgs &A, int x, int y, float d_yp, float d_ym, float d_xp,
                                            float d_xm, float3 &dv, float3 &dh) {
    const float rx = nc_rx(A, x), ry = nc_ry(A, y);
    dv = make_float3(rx * d_yp - rx * d_ym, nc_ry(A, y + 1) * d_yp - nc_ry(A, y - 1) * d_ym, d_yp - d_ym);
    dh = make_float3(nc_rx(A, x + 1) * d_xp - nc_rx(A, x - 1) * d_xm, ry * d_xp - ry * d_xm, d_xp - d_xm);
    return nc_cross3(dv, dh);
}

__device__ __forceinline__ float nc_depth(float D, float A) { return A > 0.f ? D / A : 0.f; }
// The surface at pixel p.  SURF (the *_surface entry points): the blend d = (1 - r) D / A + r m of the expected depth
// and the median depth m (2DGS's depth_ratio r), 0 where A == 0; else d = D / A, the arithmetic it always had.
template <bool SURF>
__device__ __forceinline__ float nc_surface(const NormalArgs &A, size_t p) {
    if constexpr (SURF) {
        const float a = A.A[p];
        return a > 0.f ? (1.0f - A.ratio) * (A.D[p] / a) + A.ratio * A.Md[p] : 0.f;
    } else {
        return nc_depth(A.D[p], A.A[p]);
    }
}

// 1 / |c| from |c|^2 > 0: one correctly rounded square root and one division per centre, then multiplications (with a
// division per component, 25 more per pixel, the backward took 0.059 ms at 1080p instead of 0.049).
__device__ __forceinline__ float nc_inv_norm(float l2) { return 1.0f / sqrtf(l2); }

template <bool SURF>
__global__ __launch_bounds__(256) void normal_consistency_forward_kernel(NormalArgs A) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= A.W || y >= A.H) return;
    const size_t HW = (size_t)A.H * A.W, p = (size_t)y * A.W + x;
    float3 n = make_float3(0.f, 0.f, 0.f);
    if (nc_interior(A, x, y)) {
        const size_t up = p - A.W, dn = p + A.W;
        float3 dv, dh;
        const float3 c = nc_centre(A, x, y, nc_surface<SURF>(A, dn), nc_surface<SURF>(A, up),
                                   nc_surface<SURF>(A, p + 1), nc_surface<SURF>(A, p - 1), dv, dh);
        const float l2 = c.x * c.x + c.y * c.y + c.z * c.z;
        if (l2 > 0.f) {
            const float il = nc_inv_norm(l2);
            n = make_float3(c.x * il, c.y * il, c.z * il);
        }
    }
    if (A.n_d) {
        A.n_d[p] = n.x;
        A.n_d[HW + p] = n.y;
        A.n_d[2 * HW + p] = n.z;
    }
    if (A.E) {
        const bool flat = n.x == 0.f && n.y == 0.f && n.z == 0.f;
        A.E[p] = flat ? 1.f : 1.f - A.A[p] * (A.N[p] * n.x + A.N[HW + p] * n.y + A.N[2 * HW + p] * n.z);
    }
}

void launch_normal_consistency_forward(hipStream_t s, const NormalArgs &A) {
    const dim3 grid((unsigned)((A.W + 63) / 64), (unsigned)((A.H + 3) / 4));
    if (A.Md) normal_consistency_forward_kernel<true><<<grid, dim3(64, 4), 0, s>>>(A);
    else normal_consistency_forward_kernel<false><<<grid, dim3(64, 4), 0, s>>>(A);
}

// What centre (x, y) hands to the points that made its cross product: gv = dL/d(Pt(x, y+1) - Pt(x, y-1)) and
// gh = dL/d(Pt(x+1, y) - Pt(x-1, y)), and its unit normal n (all zero for a centre on the border or with |c| = 0).
// sd: the staged d, sd[ly + 2][lx + 2] the tile pixel (lx, ly); G: dE A N at the centre.
struct NcCentreGrad {
    float3 gv, gh, n;
};
__device__ __forceinline__ NcCentreGrad nc_centre_grad(const NormalArgs &A, int x, int y, const float (*sd)[NC_DW],
                                                       int lx, int ly, float3 G) {
    NcCentreGrad r;
    r.gv = r.gh = r.n = make_float3(0.f, 0.f, 0.f);
    if (!nc_interior(A, x, y)) return r;
    float3 dv, dh;
    const float3 c = nc_centre(A, x, y, sd[ly + 3][lx + 2], sd[ly + 1][lx + 2], sd[ly + 2][lx + 3], sd[ly + 2][lx + 1],
                               dv, dh);
    const float l2 = c.x * c.x + c.y * c.y + c.z * c.z;
    if (!(l2 > 0.f)) return r;
    const float il = nc_inv_norm(l2);
    r.n = make_float3(c.x * il, c.y * il, c.z * il);
    // E = 1 - A (N . n): dL/dn = -G, dL/dc = (dL/dn - n (n . dL/dn)) / |c|
    const float nG = r.n.x * G.x + r.n.y * G.y + r.n.z * G.z;
    const float3 gc = make_float3((r.n.x * nG - G.x) * il, (r.n.y * nG - G.y) * il, (r.n.z * nG - G.z) * il);
    r.gv = nc_cross3(dh, gc);  // c = dv x dh
    r.gh = nc_cross3(gc, dv);
    return r;
}

template <bool SURF>
__global__ __launch_bounds__(256) void normal_consistency_backward_kernel(NormalArgs A) {
    __shared__ float sd[NC_DH][NC_DW];
    __shared__ float sG[3][NC_GH][NC_GW];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    const int x0 = blockIdx.x * NC_TW, y0 = blockIdx.y * NC_TH;
    const size_t HW = (size_t)A.H * A.W;
    for (int i = tid; i < NC_DH * NC_DW; i += 256) {
        const int ly = i / NC_DW, lx = i - ly * NC_DW;
        const int x = x0 - 2 + lx, y = y0 - 2 + ly;
        float d = 0.f;
        if (x >= 0 && x < A.W && y >= 0 && y < A.H) {
            d = nc_surface<SURF>(A, (size_t)y * A.W + x);
        }
        sd[ly][lx] = d;
    }
    for (int i = tid; i < NC_GH * NC_GW; i += 256) {
        const int ly = i / NC_GW, lx = i - ly * NC_GW;
        const int x = x0 - 1 + lx, y = y0 - 1 + ly;
        float3 G = make_float3(0.f, 0.f, 0.f);
        if (nc_interior(A, x, y)) {  // only interior centres are ever read
            const size_t p = (size_t)y * A.W + x;
            const float w = A.dE[p] * A.A[p];
            G = make_float3(w * A.N[p], w * A.N[HW + p], w * A.N[2 * HW + p]);
        }
        sG[0][ly][lx] = G.x;
        sG[1][ly][lx] = G.y;
        sG[2][ly][lx] = G.z;
    }
    __syncthreads();
    const int lx = threadIdx.x, x = x0 + lx;
    if (x >= A.W) return;
    const float rx = nc_rx(A, x);
    auto staged_G = [&](int gx, int gy) { return make_float3(sG[0][gy][gx], sG[1][gy][gx], sG[2][gy][gx]); };
#pragma unroll
    for (int j = 0; j < NC_ROWS; j++) {
        const int ly = threadIdx.y + 4 * j, y = y0 + ly;
        if (y >= A.H) break;
        const float ry = nc_ry(A, y);
        // this pixel is the point below centre (x, y-1), above (x, y+1), right of (x-1, y) and left of (x+1, y)
        const NcCentreGrad up = nc_centre_grad(A, x, y - 1, sd, lx, ly - 1, staged_G(lx + 1, ly));
        const NcCentreGrad dn = nc_centre_grad(A, x, y + 1, sd, lx, ly + 1, staged_G(lx + 1, ly + 2));
        const NcCentreGrad lf = nc_centre_grad(A, x - 1, y, sd, lx - 1, ly, staged_G(lx, ly + 1));
        const NcCentreGrad rt = nc_centre_grad(A, x + 1, y, sd, lx + 1, ly, staged_G(lx + 2, ly + 1));
        const NcCentreGrad me = nc_centre_grad(A, x, y, sd, lx, ly, staged_G(lx + 1, ly + 1));
        float dd = rx * up.gv.x + ry * up.gv.y + up.gv.z;
        dd -= rx * dn.gv.x + ry * dn.gv.y + dn.gv.z;
        dd += rx * lf.gh.x + ry * lf.gh.y + lf.gh.z;
        dd -= rx * rt.gh.x + ry * rt.gh.y + rt.gh.z;
        const size_t p = (size_t)y * A.W + x;
        const float a = A.A[p];
        const bool live = a > 0.f;
        if constexpr (SURF) {  // dd splits: (1 - r) of it to the expected depth D / A, r of it to the median
            const float de = (1.0f - A.ratio) * dd;
            A.dD[p] = live ? de / a : 0.f;
            A.dA[p] = live ? -de * (A.D[p] / a) / a : 0.f;
            A.dM[p] = live ? A.ratio * dd : 0.f;
        } else {
            A.dD[p] = live ? dd / a : 0.f;
            A.dA[p] = live ? -dd * sd[ly + 2][lx + 2] / a : 0.f;  // d(D / A)/dA = -d / A
        }
        const float w = nc_interior(A, x, y) ? A.dE[p] * a : 0.f;
        A.dN[p] = -w * me.n.x;
        A.dN[HW + p] = -w * me.n.y;
        A.dN[2 * HW + p] = -w * me.n.z;
    }
}

void launch_normal_consistency_backward(hipStream_t s, const NormalArgs &A) {
    const dim3 grid((unsigned)((A.W + NC_TW - 1) / NC_TW), (unsigned)((A.H + NC_TH - 1) / NC_TH));
    if (A.Md) normal_consistency_backward_kernel<true><<<grid, dim3(64, 4), 0, s>>>(A);
    else normal_consistency_backward_kernel<false><<<grid, dim3(64, 4), 0, s>>>(A);
}

}  // namespace gsr
