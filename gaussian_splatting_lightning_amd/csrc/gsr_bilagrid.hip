// gsr_bilagrid.hip -- per-image bilateral-grid colour correction: fused slice, its two gradients, and the
// total-variation regulariser (Wang et al., "Bilateral Guided Radiance Field Processing", SIGGRAPH 2024; the
// layout and definition of gsplat's lib_bilagrid, so checkpoints interchange).
//
// A grid is (12, L, Gh, Gw) fp32: channel 4r + k multiplies input colour k (k = 3: offset) into output colour r.
// Pixel (y, x) of a (3, H, W) image with value v samples the lattice trilinearly at
//     ux = (x + 0.5) / W * (Gw - 1),  uy = (y + 0.5) / H * (Gh - 1),  uz = clamp(gray(v) * (L - 1), 0, L - 1)
// and applies the sampled 3x4 affine to v.  ux and uy are rational: vertex and fraction come from integer
// arithmetic ((2x + 1)(Gw - 1) over 2W), one correctly rounded division each.
//
// slice forward / image gradient: one pass over 64x16 pixel tiles, planar coalesced reads and writes.  The tile's
//   lattice columns (a few (j, i) vertices, all L levels, 12 channels each) are staged in LDS as [vertex][level][12],
//   so a corner is three 16-B LDS reads.  The interpolation is a chain of lerps a + f (b - a): a constant grid is
//   reproduced exactly, so the identity grid returns the image bit for bit.  The image gradient recomputes the 12
//   affine values and their uz derivative in the same pass; nothing 12-channel is saved.
// grid gradient: a gather, no atomics.  A workgroup owns one (j, i) lattice column and up to 8 levels of it (12 x 8
//   register accumulators), walks the pixels of its 2x2-cell support (a slice of its rows when the support is split),
//   reduces across lanes by halving exchanges and across waves through LDS in a fixed order, and writes every vertex
//   of its column -- zeros where no pixel reaches.  Split supports go to a workspace slab per split and are summed
//   per vertex in slab order.
// TV: fixed-order block partials of the scaled squared differences (summed by the caller, as gsr_ssim.hip's), and an
//   elementwise gradient.
#include <algorithm>
#include <vector>

#include "gsr_kernels.h"

namespace gsr {

constexpr int BG_TW = 64, BG_TH = 16;
constexpr size_t BG_LDS_BYTES = 48 * 1024;  // above this the tile's columns are read from global memory (L2) instead
constexpr int BG_LC = 8;                    // levels per grid-gradient workgroup
constexpr int BG_SPLIT_TARGET = 1024;       // grid-gradient workgroups wanted (4 per CU)
constexpr int BG_SPLIT_MIN_PX = 1024;       // ... of at least this many support pixels each

// Lower vertex and fraction in [0, 1) of pixel centre p of n along a lattice axis of G vertices.  i0 <= G - 2.
__device__ __forceinline__ void bg_axis(int p, int n, int G, int &i0, float &f) {
    const int num = (2 * p + 1) * (G - 1), den = 2 * n;  // (G == 1: 0)
    i0 = num / den;
    f = (float)(num - i0 * den) / (float)den;
}

__device__ __forceinline__ float bg_gray(float v0, float v1, float v2) {
    return fmaf(0.114f, v2, fmaf(0.587f, v1, 0.299f * v0));
}

__device__ __forceinline__ float bg_uz(float gray, int L) { return fminf(fmaxf(gray * (float)(L - 1), 0.f), (float)(L - 1)); }

// Vertex columns a 64- (or 16-) pixel tile edge can touch: its lower vertices span floor((T-1)(G-1)/n) + 1 values.
static int bg_tile_vertices(int T, int n, int G) {
    return (int)std::min<int64_t>(G, (int64_t)(T - 1) * (G - 1) / n + 3);
}

struct BgCorner {
    float a[12];
};

template <bool LDS>
__device__ __forceinline__ BgCorner bg_load(const float *__restrict__ grid, const float4 *lds, const BgShape &S,
                                            int nvx, int ix_lo, int iy_lo, int l, int j, int i) {
    BgCorner c;
    if (LDS) {
        const float4 *p = lds + ((size_t)((j - iy_lo) * nvx + (i - ix_lo)) * S.L + l) * 3;
        const float4 q0 = p[0], q1 = p[1], q2 = p[2];
        c.a[0] = q0.x, c.a[1] = q0.y, c.a[2] = q0.z, c.a[3] = q0.w;
        c.a[4] = q1.x, c.a[5] = q1.y, c.a[6] = q1.z, c.a[7] = q1.w;
        c.a[8] = q2.x, c.a[9] = q2.y, c.a[10] = q2.z, c.a[11] = q2.w;
    } else {
        const size_t cs = (size_t)S.L * S.Gh * S.Gw;
        const float *p = grid + ((size_t)l * S.Gh + j) * S.Gw + i;
#pragma unroll
        for (int k = 0; k < 12; k++) c.a[k] = p[k * cs];
    }
    return c;
}

__device__ __forceinline__ void bg_lerp(BgCorner &a, const BgCorner &b, float f) {
#pragma unroll
    for (int k = 0; k < 12; k++) a.a[k] = fmaf(f, b.a[k] - a.a[k], a.a[k]);
}

// BWD = false: out = slice(image).  BWD = true: out = dL/dimage from dout = dL/dslice.
template <bool LDS, bool BWD>
__global__ __launch_bounds__(256) void bg_slice_kernel(BgShape S, BgBatch Bt, const float *__restrict__ grids,
                                                       const float *__restrict__ image,
                                                       const float *__restrict__ dout, float *__restrict__ out) {
    extern __shared__ float4 bg_lds[];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * BG_TW, y0 = blockIdx.y * BG_TH, b = blockIdx.z;
    const size_t gsz = (size_t)12 * S.L * S.Gh * S.Gw, plane = (size_t)S.H * S.W;
    const float *grid = grids + (size_t)Bt.g[b] * gsz;
    const float *img = image + (size_t)(Bt.b0 + b) * 3 * plane;
    int ix_lo, iy_lo, nvx = 0;
    {
        float f;
        int hi;
        bg_axis(x0, S.W, S.Gw, ix_lo, f);
        bg_axis(min(x0 + BG_TW, S.W) - 1, S.W, S.Gw, hi, f);
        nvx = min(hi + 1, S.Gw - 1) - ix_lo + 1;
        bg_axis(y0, S.H, S.Gh, iy_lo, f);
        if (LDS) {
            bg_axis(min(y0 + BG_TH, S.H) - 1, S.H, S.Gh, hi, f);
            const int nvy = min(hi + 1, S.Gh - 1) - iy_lo + 1;
            const int n = nvy * nvx * S.L * 12;
            float *s = reinterpret_cast<float *>(bg_lds);
            for (int e = tid; e < n; e += 256) {  // vertex x fastest: contiguous in global memory
                const int vx = e % nvx, r1 = e / nvx, vy = r1 % nvy, r2 = r1 / nvy, l = r2 % S.L, c = r2 / S.L;
                s[((size_t)(vy * nvx + vx) * S.L + l) * 12 + c] =
                    grid[(((size_t)c * S.L + l) * S.Gh + (iy_lo + vy)) * S.Gw + (ix_lo + vx)];
            }
            __syncthreads();
        }
    }
    const int x = x0 + (tid & (BG_TW - 1));
    if (x >= S.W) return;
    int i0;
    float fx;
    bg_axis(x, S.W, S.Gw, i0, fx);
    const int i1 = min(i0 + 1, S.Gw - 1);
#pragma unroll 1
    for (int ry = tid / BG_TW; ry < BG_TH; ry += 256 / BG_TW) {
        const int y = y0 + ry;
        if (y >= S.H) break;
        int j0;
        float fy;
        bg_axis(y, S.H, S.Gh, j0, fy);
        const int j1 = min(j0 + 1, S.Gh - 1);
        const size_t pid = (size_t)y * S.W + x;
        const float v0 = img[pid], v1 = img[pid + plane], v2 = img[pid + 2 * plane];
        const float gray = bg_gray(v0, v1, v2);
        const float uz = bg_uz(gray, S.L);
        const int l0 = max(min((int)uz, S.L - 2), 0), l1 = min(l0 + 1, S.L - 1);
        const float fz = uz - (float)l0;
        BgCorner P0 = bg_load<LDS>(grid, bg_lds, S, nvx, ix_lo, iy_lo, l0, j0, i0);
        bg_lerp(P0, bg_load<LDS>(grid, bg_lds, S, nvx, ix_lo, iy_lo, l0, j0, i1), fx);
        {
            BgCorner q = bg_load<LDS>(grid, bg_lds, S, nvx, ix_lo, iy_lo, l0, j1, i0);
            bg_lerp(q, bg_load<LDS>(grid, bg_lds, S, nvx, ix_lo, iy_lo, l0, j1, i1), fx);
            bg_lerp(P0, q, fy);
        }
        BgCorner P1 = bg_load<LDS>(grid, bg_lds, S, nvx, ix_lo, iy_lo, l1, j0, i0);
        bg_lerp(P1, bg_load<LDS>(grid, bg_lds, S, nvx, ix_lo, iy_lo, l1, j0, i1), fx);
        {
            BgCorner q = bg_load<LDS>(grid, bg_lds, S, nvx, ix_lo, iy_lo, l1, j1, i0);
            bg_lerp(q, bg_load<LDS>(grid, bg_lds, S, nvx, ix_lo, iy_lo, l1, j1, i1), fx);
            bg_lerp(P1, q, fy);
        }
        float *o = out + (size_t)(Bt.b0 + b) * 3 * plane + pid;
        if (!BWD) {
            bg_lerp(P0, P1, fz);
#pragma unroll
            for (int r = 0; r < 3; r++)
                o[r * plane] = fmaf(P0.a[4 * r], v0, fmaf(P0.a[4 * r + 1], v1, fmaf(P0.a[4 * r + 2], v2, P0.a[4 * r + 3])));
        } else {
            const float *go = dout + (size_t)(Bt.b0 + b) * 3 * plane + pid;
            float d0 = 0.f, d1 = 0.f, d2 = 0.f, dz = 0.f;
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const float g = go[r * plane];
                const float z0 = P1.a[4 * r] - P0.a[4 * r], z1 = P1.a[4 * r + 1] - P0.a[4 * r + 1],
                            z2 = P1.a[4 * r + 2] - P0.a[4 * r + 2], z3 = P1.a[4 * r + 3] - P0.a[4 * r + 3];
                dz = fmaf(g, fmaf(z0, v0, fmaf(z1, v1, fmaf(z2, v2, z3))), dz);  // dout_r . dA/duz . (v, 1)
                d0 = fmaf(g, fmaf(fz, z0, P0.a[4 * r]), d0);
                d1 = fmaf(g, fmaf(fz, z1, P0.a[4 * r + 1]), d1);
                d2 = fmaf(g, fmaf(fz, z2, P0.a[4 * r + 2]), d2);
            }
            if (gray > 0.f && gray < 1.f) {  // uz = gray (L - 1) unclamped
                dz *= (float)(S.L - 1);
                d0 = fmaf(0.299f, dz, d0);
                d1 = fmaf(0.587f, dz, d1);
                d2 = fmaf(0.114f, dz, d2);
            }
            o[0] = d0, o[plane] = d1, o[2 * plane] = d2;
        }
    }
}

// N values per lane summed over the wave: while N halves evenly each exchange trades half of the values (the lane
// keeps N / 2 sums of pairs), then the rest are butterflied.  The lane ends with the wave's sums of elements
// base .. base + bg_reduced(N) - 1; every step adds the same two operands in both partners, so the order is fixed.
template <int N, int MASK>
__device__ __forceinline__ void bg_wave_reduce(float *a, int lane, int &base) {
    if constexpr (MASK > 0) {
        if constexpr (N % 2 == 0 && N >= 6) {
            constexpr int n = N / 2;
            const bool up = (lane & MASK) != 0;
#pragma unroll
            for (int i = 0; i < n; i++) {
                const float send = up ? a[i] : a[i + n], keep = up ? a[i + n] : a[i];
                a[i] = keep + __shfl_xor(send, MASK);
            }
            base += up ? n : 0;
            bg_wave_reduce<n, MASK / 2>(a, lane, base);
        } else {
#pragma unroll
            for (int i = 0; i < N; i++) a[i] += __shfl_xor(a[i], MASK);
            bg_wave_reduce<N, MASK / 2>(a, lane, base);
        }
    }
}
constexpr int bg_reduced(int N, int MASK) {
    return MASK == 0 ? N : (N % 2 == 0 && N >= 6) ? bg_reduced(N / 2, MASK / 2) : bg_reduced(N, MASK / 2);
}

// Pixel range [lo, hi] (maybe a little wider) with hat((p + 0.5) / n * (G - 1) - i) > 0.
__device__ __forceinline__ void bg_support(int i, int n, int G, int &lo, int &hi) {
    lo = 0, hi = n - 1;
    if (G > 1) {
        lo = max(0, (int)((int64_t)(i - 1) * n / (G - 1)) - 1);
        hi = min(n - 1, (int)((int64_t)(i + 1) * n / (G - 1)));
    }
}

// dL/dgrid of one image.  blockIdx.x: lattice column j * Gw + i; blockIdx.y: split of the support's rows;
// blockIdx.z: chunk of LC levels.  dst is one grid (12, L, Gh, Gw), blockIdx.y * split_stride floats further on for
// each split; accumulate adds to what dst holds (a later image of the same grid).
template <int LC>
__global__ __launch_bounds__(256) void bg_dgrid_kernel(BgShape S, const float *__restrict__ img,
                                                       const float *__restrict__ dout, float *dst,
                                                       size_t split_stride, int accumulate) {
    constexpr int NA = LC * 12, NR = bg_reduced(NA, 32);
    __shared__ float s_red[4][NA];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x % S.Gw, j = blockIdx.x / S.Gw, lbase = blockIdx.z * LC;
    const size_t plane = (size_t)S.H * S.W;
    int xlo, xhi, ylo, yhi;
    bg_support(i, S.W, S.Gw, xlo, xhi);
    bg_support(j, S.H, S.Gh, ylo, yhi);
    const int rows_per = (yhi - ylo + (int)gridDim.y) / (int)gridDim.y;  // ceil(rows / splits)
    const int r0 = ylo + blockIdx.y * rows_per, r1 = min(yhi + 1, r0 + rows_per);
    const int ncols = xhi - xlo + 1, npx = max(r1 - r0, 0) * ncols;
    const float inv_dx = 1.f / (float)(2 * S.W), inv_dy = 1.f / (float)(2 * S.H);
    float acc[NA];
#pragma unroll
    for (int e = 0; e < NA; e++) acc[e] = 0.f;
    for (int p = tid; p < npx; p += 256) {
        const int ry = p / ncols, x = xlo + (p - ry * ncols), y = r0 + ry;
        const float tx = (float)((2 * x + 1) * (S.Gw - 1) - i * 2 * S.W) * inv_dx;
        const float ty = (float)((2 * y + 1) * (S.Gh - 1) - j * 2 * S.H) * inv_dy;
        const float wxy = fmaxf(0.f, 1.f - fabsf(tx)) * fmaxf(0.f, 1.f - fabsf(ty));
        const size_t pid = (size_t)y * S.W + x;
        const float v0 = img[pid], v1 = img[pid + plane], v2 = img[pid + 2 * plane];
        const float uz = bg_uz(bg_gray(v0, v1, v2), S.L) - (float)lbase;
        float pr[12];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const float g = dout[pid + r * plane] * wxy;
            pr[4 * r] = g * v0, pr[4 * r + 1] = g * v1, pr[4 * r + 2] = g * v2, pr[4 * r + 3] = g;
        }
#pragma unroll
        for (int l = 0; l < LC; l++) {
            const float wl = fmaxf(0.f, 1.f - fabsf(uz - (float)l));
#pragma unroll
            for (int c = 0; c < 12; c++) acc[l * 12 + c] = fmaf(wl, pr[c], acc[l * 12 + c]);
        }
    }
    int base = 0;
    bg_wave_reduce<NA, 32>(acc, lane, base);
#pragma unroll
    for (int e = 0; e < NR; e++) s_red[wave][base + e] = acc[e];  // (the lanes that share a base hold the same sums)
    __syncthreads();
    if (tid < NA) {
        const int l = lbase + tid / 12, c = tid % 12;
        if (l < S.L) {
            const float v = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
            float *o = dst + blockIdx.y * split_stride + (((size_t)c * S.L + l) * S.Gh + j) * S.Gw + i;
            *o = accumulate ? *o + v : v;
        }
    }
}

// dst[e] (+)= slab 0 + slab 1 + ... in slab order
__global__ __launch_bounds__(256) void bg_sum_splits_kernel(int n, int nsplit, const float *__restrict__ slabs,
                                                            float *dst, int accumulate) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float v = slabs[e];
    for (int s = 1; s < nsplit; s++) v += slabs[(size_t)s * n + e];
    dst[e] = accumulate ? dst[e] + v : v;
}

static int bg_level_chunk(int L) { return L == 1 ? 1 : L <= 4 ? 4 : BG_LC; }

// Splits of a column's support rows: a function of the shapes alone, so that a call always sums in the same order.
int bilagrid_splits(const BgShape &S) {
    const int chunks = div_up(S.L, bg_level_chunk(S.L));
    const int64_t cols = (int64_t)S.Gh * S.Gw * chunks;
    const int64_t sup_h = S.Gh == 1 ? S.H : std::min<int64_t>(S.H, 2 * (int64_t)S.H / (S.Gh - 1) + 2);
    const int64_t sup_w = S.Gw == 1 ? S.W : std::min<int64_t>(S.W, 2 * (int64_t)S.W / (S.Gw - 1) + 2);
    int64_t s = (BG_SPLIT_TARGET + cols - 1) / cols;
    s = std::min(s, sup_h * sup_w / BG_SPLIT_MIN_PX);
    s = std::min<int64_t>(std::min(s, sup_h), 65535);
    return (int)std::max<int64_t>(s, 1);
}

size_t bilagrid_workspace_bytes(const BgShape &S) {
    const int s = bilagrid_splits(S);
    return s > 1 ? (size_t)s * 12 * S.L * S.Gh * S.Gw * sizeof(float) : 0;
}

static size_t bg_tile_lds_bytes(const BgShape &S) {
    return (size_t)bg_tile_vertices(BG_TW, S.W, S.Gw) * bg_tile_vertices(BG_TH, S.H, S.Gh) * S.L * 12 * sizeof(float);
}

template <bool BWD>
static void bg_launch_slice(hipStream_t s, const BgShape &S, int B, const int32_t *idx, const float *grids,
                            const float *image, const float *dout, float *out) {
    const size_t lds = bg_tile_lds_bytes(S);
    for (int b0 = 0; b0 < B; b0 += BG_MAX_BATCH) {
        BgBatch Bt;
        Bt.b0 = b0;
        const int n = std::min(B - b0, BG_MAX_BATCH);
        for (int k = 0; k < BG_MAX_BATCH; k++) Bt.g[k] = idx[b0 + std::min(k, n - 1)];
        const dim3 grid(div_up(S.W, BG_TW), div_up(S.H, BG_TH), n), block(256);
        if (lds <= BG_LDS_BYTES)
            bg_slice_kernel<true, BWD><<<grid, block, lds, s>>>(S, Bt, grids, image, dout, out);
        else
            bg_slice_kernel<false, BWD><<<grid, block, 0, s>>>(S, Bt, grids, image, dout, out);
    }
}

void launch_bilagrid_slice_forward(hipStream_t s, const BgShape &S, int B, const int32_t *idx, const float *grids,
                                   const float *image, float *out) {
    bg_launch_slice<false>(s, S, B, idx, grids, image, nullptr, out);
}

void launch_bilagrid_slice_backward_image(hipStream_t s, const BgShape &S, int B, const int32_t *idx,
                                          const float *grids, const float *image, const float *dout, float *dimage) {
    bg_launch_slice<true>(s, S, B, idx, grids, image, dout, dimage);
}

// dgrids (num grids) is written whole: zeros first, then image after image in order, each into its grid.
hipError_t launch_bilagrid_slice_backward_grid(hipStream_t s, const BgShape &S, int num, int B, const int32_t *idx,
                                               const float *image, const float *dout, float *dgrids, float *workspace) {
    const size_t gsz = (size_t)12 * S.L * S.Gh * S.Gw, plane = (size_t)S.H * S.W;
    const hipError_t e = hipMemsetAsync(dgrids, 0, (size_t)num * gsz * sizeof(float), s);
    if (e != hipSuccess) return e;
    const int nsplit = bilagrid_splits(S), LC = bg_level_chunk(S.L);
    const dim3 grid(S.Gh * S.Gw, nsplit, div_up(S.L, LC)), block(256);
    std::vector<char> seen(num, 0);
    for (int b = 0; b < B; b++) {
        float *dst = dgrids + (size_t)idx[b] * gsz;
        const int acc = seen[idx[b]];
        seen[idx[b]] = 1;
        float *to = nsplit > 1 ? workspace : dst;
        const size_t stride = nsplit > 1 ? gsz : 0;
        const int acc1 = nsplit > 1 ? 0 : acc;
        const float *img = image + (size_t)b * 3 * plane, *go = dout + (size_t)b * 3 * plane;
        if (LC == 1)
            bg_dgrid_kernel<1><<<grid, block, 0, s>>>(S, img, go, to, stride, acc1);
        else if (LC == 4)
            bg_dgrid_kernel<4><<<grid, block, 0, s>>>(S, img, go, to, stride, acc1);
        else
            bg_dgrid_kernel<BG_LC><<<grid, block, 0, s>>>(S, img, go, to, stride, acc1);
        if (nsplit > 1)
            bg_sum_splits_kernel<<<div_up(gsz, 256), 256, 0, s>>>((int)gsz, nsplit, workspace, dst, acc);
    }
    return hipSuccess;
}

// ---- total variation ----
// tv = (1 / num) sum over axes of (sum of squared first differences) / (12 (n - 1) (the other two sizes)).
constexpr int BG_TV_MAX_BLOCKS = 1024;

struct BgTv {
    int L, Gh, Gw;
    float cz, cy, cx;  // 1 / (num 12 (n - 1) others), 0 for an axis of size 1
    uint32_t total;    // num 12 L Gh Gw (the entry points refuse more than 2^31 - 1)
};

static BgTv bg_tv(int num, int L, int Gh, int Gw) {
    BgTv t{L, Gh, Gw, 0.f, 0.f, 0.f, (uint32_t)((size_t)num * 12 * L * Gh * Gw)};
    const double k = 12.0 * num;
    if (L > 1) t.cz = (float)(1.0 / (k * (L - 1) * Gh * Gw));
    if (Gh > 1) t.cy = (float)(1.0 / (k * L * (Gh - 1) * Gw));
    if (Gw > 1) t.cx = (float)(1.0 / (k * L * Gh * (Gw - 1)));
    return t;
}

size_t bilagrid_tv_num_partials(int num, int L, int Gh, int Gw) {
    return std::min<size_t>(BG_TV_MAX_BLOCKS, div_up((size_t)num * 12 * L * Gh * Gw, 256 * 8));
}

__global__ __launch_bounds__(256) void bg_tv_fwd_kernel(BgTv T, const float *__restrict__ g,
                                                        float *__restrict__ partial) {
    __shared__ float s_red[4];
    const uint32_t sy = T.Gw, sz = (uint32_t)T.Gh * T.Gw;
    float acc = 0.f;
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < T.total; e += gridDim.x * 256) {
        const int i = (int)(e % sy), j = (int)(e / sy % T.Gh), l = (int)(e / sz % T.L);
        const float v = g[e];
        float a = 0.f;
        if (i + 1 < T.Gw) {
            const float d = g[e + 1] - v;
            a = T.cx * d * d;
        }
        if (j + 1 < T.Gh) {
            const float d = g[e + sy] - v;
            a = fmaf(T.cy * d, d, a);
        }
        if (l + 1 < T.L) {
            const float d = g[e + sz] - v;
            a = fmaf(T.cz * d, d, a);
        }
        acc += a;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

__global__ __launch_bounds__(256) void bg_tv_bwd_kernel(BgTv T, const float *__restrict__ g,
                                                        const float *__restrict__ dL_dtv, float *__restrict__ dg) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= T.total) return;
    const uint32_t sy = T.Gw, sz = (uint32_t)T.Gh * T.Gw;
    const int i = (int)(e % sy), j = (int)(e / sy % T.Gh), l = (int)(e / sz % T.L);
    const float v = g[e];
    float a = 0.f;
    if (i > 0) a = fmaf(T.cx, v - g[e - 1], a);
    if (i + 1 < T.Gw) a = fmaf(T.cx, v - g[e + 1], a);
    if (j > 0) a = fmaf(T.cy, v - g[e - sy], a);
    if (j + 1 < T.Gh) a = fmaf(T.cy, v - g[e + sy], a);
    if (l > 0) a = fmaf(T.cz, v - g[e - sz], a);
    if (l + 1 < T.L) a = fmaf(T.cz, v - g[e + sz], a);
    dg[e] = 2.f * dL_dtv[0] * a;
}

void launch_bilagrid_tv_forward(hipStream_t s, int num, int L, int Gh, int Gw, const float *grids, float *partial) {
    const BgTv T = bg_tv(num, L, Gh, Gw);
    bg_tv_fwd_kernel<<<(unsigned)bilagrid_tv_num_partials(num, L, Gh, Gw), 256, 0, s>>>(T, grids, partial);
}

void launch_bilagrid_tv_backward(hipStream_t s, int num, int L, int Gh, int Gw, const float *grids,
                                 const float *dL_dtv, float *dgrids) {
    const BgTv T = bg_tv(num, L, Gh, Gw);
    bg_tv_bwd_kernel<<<div_up(T.total, 256), 256, 0, s>>>(T, grids, dL_dtv, dgrids);
}

}  // namespace gsr
