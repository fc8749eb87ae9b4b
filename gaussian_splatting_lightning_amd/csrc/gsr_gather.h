// Which of a Gaussian's instance rows the backward's per-Gaussian gathers add, decided in one place: the 40-B rows
// (preprocess_bwd_kernel), the 8-B abs rows (abs_gather_kernel) and the feature rows (feat_gather_kernel) must take
// the same decisions, or their sums silently disagree.  Each kernel keeps its own row loads and additions.
#pragma once
#include "gsr_kernels.h"

namespace gsr {

// The live flag of Gaussian g (0: the composite stored no non-zero row of it, so its sums are zero), trusted only when
// the validity word says the last composite marked the flags
template <typename I>
__device__ __forceinline__ bool gather_live(const GatherSrc &s, I g) {
    return !s.live || !*s.live_valid || s.live[g];
}
// Whether Gaussian g's rows are gathered at all: a positive radius and its live flag
template <typename I>
__device__ __forceinline__ bool gather_wanted(const GatherSrc &s, I g, int radius) {
    return radius > 0 && gather_live(s, g);
}
// Instances k0 .. k0 + 3 of a Gaussian with cnt instances from expansion index start: use[j] when the instance exists
// and the forward composite loaded it (inv != INV_NONE: it has a row).  The four inv loads are unconditional (index
// clamped to the last instance) so that they are in flight together.
__device__ __forceinline__ void inv_use4(const GatherSrc &s, uint32_t start, uint32_t k0, uint32_t cnt, bool (&use)[4]) {
    uint32_t iv[4];
#pragma unroll
    for (int j = 0; j < 4; j++) iv[j] = s.inv[start + min(k0 + j, cnt - 1)];
#pragma unroll
    for (int j = 0; j < 4; j++) use[j] = k0 + j < cnt && iv[j] != INV_NONE;
}

}  // namespace gsr
