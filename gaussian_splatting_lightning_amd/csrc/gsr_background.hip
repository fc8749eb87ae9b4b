// gsr_background.hip -- the background's gradients (gsr_composite_ext) and the forward of a scene without Gaussians.
//
// The forward composites out_color_c = C_c + T_final * B_c over a background B (three floats, or a (3,H,W) image), so
//   dL/dB_c(pix) = T_final(pix) * dL/dout_color_c(pix)     and     dL/dbg_c = sum over the pixels of that
// for the 3-vector.  One pass reads final_T and dL_dpix once (16 B per pixel), writes the image gradient and / or one
// partial sum per workgroup and channel; a second one-workgroup launch adds the partials in index order.  Which pixel
// goes to which thread, workgroup and partial depends only on the pixel count, and every sum is a fixed tree (four
// pixels pairwise per thread, the wave's DPP tree, the four waves through LDS, the partials strided over one
// workgroup): no float atomics, the same bits on every call.  HBM-bound: 16 B loads and stores per lane where the
// planes are 16-B aligned (the pixel-to-thread map is the same either way, so alignment never changes a result), at
// most 2048 workgroups (8 per CU) that stride over the rest.
#include <algorithm>

#include "gsr_kernels.h"

namespace gsr {

constexpr int BG_THREADS = 256, BG_PIX = 4, BG_CHUNK = BG_THREADS * BG_PIX;  // pixels of one workgroup pass
constexpr uint32_t BG_MAX_BLOCKS = 2048;

static uint32_t background_blocks(size_t HW) {
    return std::max(1u, std::min(div_up(HW, BG_CHUNK), BG_MAX_BLOCKS));
}
size_t background_partials_bytes(size_t HW) { return sizeof(float) * 3 * background_blocks(HW); }

// the workgroup's sum of one value per thread: wave tree, then the four waves in order; valid in thread 0
__device__ __forceinline__ float bg_block_sum(float v, float *s_w) {
    const float ws = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = ws;
    __syncthreads();
    return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// VEC: HW is a multiple of 4 and every plane is 16-B aligned.  final_T null: T = 1 everywhere (no Gaussian).
template <bool VEC>
__global__ __launch_bounds__(BG_THREADS) void background_grad_kernel(size_t HW, const float *__restrict__ final_T,
                                                                     const float *__restrict__ dL_dpix,
                                                                     float *__restrict__ dimg,
                                                                     float *__restrict__ partials) {
#pragma clang fp contract(off)  // the image gradient is one rounded product, and the sums add exactly those values
    __shared__ float s_w[3][4];
    float acc[3] = {0.f, 0.f, 0.f};
    for (size_t base = (size_t)blockIdx.x * BG_CHUNK; base < HW; base += (size_t)gridDim.x * BG_CHUNK) {
        const size_t i0 = base + (size_t)threadIdx.x * BG_PIX;  // this thread's pixels [i0, i0 + 4)
        float t[BG_PIX], v[3][BG_PIX];
        if (VEC) {
            const bool in = i0 < HW;  // whole quads: HW % 4 == 0
            const float4 one = make_float4(1.f, 1.f, 1.f, 1.f), zero = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 t4 = !in ? zero : final_T ? *reinterpret_cast<const float4 *>(final_T + i0) : one;
            t[0] = t4.x; t[1] = t4.y; t[2] = t4.z; t[3] = t4.w;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float4 d = in ? *reinterpret_cast<const float4 *>(dL_dpix + c * HW + i0) : zero;
                v[c][0] = t[0] * d.x; v[c][1] = t[1] * d.y; v[c][2] = t[2] * d.z; v[c][3] = t[3] * d.w;
                if (dimg && in)
                    *reinterpret_cast<float4 *>(dimg + c * HW + i0) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
            }
        } else {
#pragma unroll
            for (int q = 0; q < BG_PIX; q++) t[q] = i0 + q >= HW ? 0.f : final_T ? final_T[i0 + q] : 1.f;
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int q = 0; q < BG_PIX; q++) {
                    const bool in = i0 + q < HW;
                    v[c][q] = t[q] * (in ? dL_dpix[c * HW + i0 + q] : 0.f);
                    if (dimg && in) dimg[c * HW + i0 + q] = v[c][q];
                }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) acc[c] += (v[c][0] + v[c][1]) + (v[c][2] + v[c][3]);
    }
    if (!partials) return;  // uniform: only the image gradient was asked for
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float sum = bg_block_sum(acc[c], s_w[c]);
        if (threadIdx.x == 0) partials[(size_t)c * gridDim.x + blockIdx.x] = sum;
    }
}

// dbg[c] = the partials of channel c (nb each) in a fixed order: thread t adds t, t + 256, ..., then the workgroup tree
__global__ __launch_bounds__(BG_THREADS) void background_reduce_kernel(const float *__restrict__ partials, uint32_t nb,
                                                                       float *__restrict__ dbg) {
    __shared__ float s_w[3][4];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float a = 0.f;
        for (uint32_t i = threadIdx.x; i < nb; i += BG_THREADS) a += partials[(size_t)c * nb + i];
        const float sum = bg_block_sum(a, s_w[c]);
        if (threadIdx.x == 0) dbg[c] = sum;
    }
}

void launch_background_grad(hipStream_t s, size_t HW, const float *final_T, const float *dL_dpix, float *dimg,
                            float *dbg, float *partials) {
    if (HW == 0 || (!dimg && !dbg)) return;
    const uint32_t nb = background_blocks(HW);
    const uintptr_t al = (uintptr_t)final_T | (uintptr_t)dL_dpix | (uintptr_t)dimg;
    float *part = dbg ? partials : nullptr;
    if (HW % 4 == 0 && (al & 15) == 0)
        background_grad_kernel<true><<<nb, BG_THREADS, 0, s>>>(HW, final_T, dL_dpix, dimg, part);
    else
        background_grad_kernel<false><<<nb, BG_THREADS, 0, s>>>(HW, final_T, dL_dpix, dimg, part);
    if (dbg) background_reduce_kernel<<<1, BG_THREADS, 0, s>>>(partials, nb, dbg);
}

// out_color = the background of every pixel, out_alpha = 0: what the composite writes where no Gaussian reaches
__global__ __launch_bounds__(BG_THREADS) void background_fill_kernel(size_t HW, const float *__restrict__ bg,
                                                                     const float *__restrict__ bg_image,
                                                                     float *__restrict__ out_color,
                                                                     float *__restrict__ out_alpha) {
    for (size_t i = (size_t)blockIdx.x * BG_THREADS + threadIdx.x; i < HW; i += (size_t)gridDim.x * BG_THREADS) {
#pragma unroll
        for (int c = 0; c < 3; c++) out_color[c * HW + i] = bg_image ? bg_image[c * HW + i] : bg[c];
        if (out_alpha) out_alpha[i] = 0.f;
    }
}

void launch_background_fill(hipStream_t s, size_t HW, const float *bg, const float *bg_image, float *out_color,
                            float *out_alpha) {
    if (HW == 0) return;
    const uint32_t nb = std::max(1u, std::min(div_up(HW, BG_THREADS), BG_MAX_BLOCKS));
    background_fill_kernel<<<nb, BG_THREADS, 0, s>>>(HW, bg, bg_image, out_color, out_alpha);
}

}  // namespace gsr
