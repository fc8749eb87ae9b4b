// gsr_replay.h -- what every replay of the colour forward shares (the feature kernels of gsr_features.hip, the
// contribution walk of gsr_contrib.hip): a batch's record staging and the composite's alpha decision, in one place so
// that the replays take the pairs the colour forward took.
#pragma once
#include "gsr_gather.h"

namespace gsr {

constexpr int FEAT_BATCH = 32;

// One batch's records, Gaussian ids and strip masks: lane j < cnt stages the instance at sorted position s0 + j * step
// (step = +1 front to back, -1 back to front).  Returns the lane's 4-bit strip mask (cell_mask: conservative, a strip
// without its bit holds no pixel that passes the alpha test).
__device__ __forceinline__ uint32_t feat_stage(const GRec *__restrict__ rec, const uint32_t *__restrict__ point_list,
                                               uint32_t s_me, bool mine, int lane, FwdRec *s_rec, uint32_t *s_gid,
                                               bool strip_exact, float row0, float col0, float4 &raw_a, float4 &raw_b) {
    uint32_t m = 0;
    if (mine) {
        const uint32_t gid = point_list[s_me];
        s_gid[lane] = gid;
        raw_a = rec[gid].a;
        raw_b = rec[gid].b;
        s_rec[lane].a = stage_rec_a(raw_a);
        s_rec[lane].b = stage_rec_b(raw_b);
        m = cell_mask(strip_exact, raw_a, raw_b, row0, col0);
    }
    return m;
}

// The composite's alpha decision for one (pixel, instance) pair: power <= 0 and alpha >= 1/255.  GUARD ("guard" knob):
// the forward's guarded decision (gsr_common.h) -- a pair whose alpha lies in the band around 1/255 is re-decided from
// the oracle's own arithmetic on the raw record, exactly as render_fwd_v6_kernel / render_bwd_v5_kernel do, so the
// replay takes the pairs the guarded colour forward took.
template <bool GUARD>
__device__ __forceinline__ bool feat_alpha_pass(float power2, float alpha, const GRec *__restrict__ rec, uint32_t gid,
                                                float pfx, float pfy) {
    if constexpr (GUARD) {
        if (!(power2 <= 0.0f) || !(alpha >= GUARD_A_LO)) return false;
        if (alpha >= GUARD_A_HI) return true;
        return guard_alpha_pass(rec, gid, pfx, pfy);  // rare
    } else {
        return power2 <= 0.0f && !(alpha < 1.0f / 255.0f);
    }
}

}  // namespace gsr
