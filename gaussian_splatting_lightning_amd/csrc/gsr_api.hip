// gsr_api.hip -- the extern "C" boundary declared in include/gsrast.h.
//
// Mirrors the orchestration of the reference's CUDA entry points (rasterize_points.cu
// RasterizeGaussiansCUDA / RasterizeGaussiansBackwardCUDA / markVisible and
// rasterizer_impl.cu Rasterizer::forward/backward, SURVEY.md §2.1, [U]) with the MI355X stage list of
// preprocess -> depth sort -> instance scan -> one 8-byte readback -> expand -> tile sort ->
// ranges -> composite; backward: reverse composite -> big-Gaussian reduce -> preprocess backward.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>

#include <immintrin.h>
#include <chrono>
#include <string>
#include <vector>

#include "gsr_kernels.h"
#include "gsrast.h"

using namespace gsr;

namespace {

std::mutex g_tune_mu;  // stamp_buffer's

// The knob table (gsr_knobs.def): names and built-in defaults, and per knob a value with its "set" flag.
struct KnobInfo {
    const char *name;
    int def;
};
constexpr KnobInfo kKnobs[K_COUNT] = {
#define GSR_KNOB(name, def, cls, doc) {#name, (def)},
#include "gsr_knobs.def"
#undef GSR_KNOB
};
std::atomic<int> g_knob_value[K_COUNT];
std::atomic<bool> g_knob_set[K_COUNT];
// read-only statistic, read through gsr_get_tuning: the last forward's depth-sort passes, 0 on the bucket path
constexpr const char *kStatDepthPasses = "stat_depth_passes";
std::atomic<int> g_stat_depth_passes{GSR_TUNING_UNSET};

int find_knob(const char *name) {
    for (int k = 0; name && k < K_COUNT; k++)
        if (!strcmp(kKnobs[k].name, name)) return k;
    return -1;
}

}  // namespace

int gsr::tuning(Knob k) {
    return g_knob_set[k].load(std::memory_order_relaxed) ? g_knob_value[k].load(std::memory_order_relaxed) : kKnobs[k].def;
}

uint4 *gsr::stamp_buffer(int which) {
    static uint4 *buf[4] = {nullptr, nullptr, nullptr, nullptr};
    std::lock_guard<std::mutex> lk(g_tune_mu);
    if (which < 0 || which > 3) return nullptr;
    if (!buf[which] && hipMalloc(&buf[which], sizeof(uint4) * STAMP_SLOTS) == hipSuccess)
        (void)hipMemset(buf[which], 0, sizeof(uint4) * STAMP_SLOTS);
    return buf[which];
}

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define GSR_HIP(x)                                                                                  \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) {                                                                     \
            (void)hipGetLastError(); /* do not leave a sticky error for the caller's runtime */     \
            return fail(GSR_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));               \
        }                                                                                           \
    } while (0)

// ---- per-stage profiling --------------------------------------------------------------------------
enum Stage {
    ST_PREPROCESS = 0,
    ST_DEPTH_SORT,
    ST_SCAN,
    ST_READBACK,
    ST_EXPAND,
    ST_TILE_SORT,
    ST_RANGES,
    ST_RENDER_FWD,
    ST_RENDER_BWD,
    ST_BIG_REDUCE,
    ST_PREPROCESS_BWD,
    ST_SH_VIEWS,
    ST_BK_COUNT,
    ST_BK_SCATTER,
    ST_SEG_SORT,
    ST_ADAM_SH,
    ST_BACKGROUND_GRAD,
    ST_DIST_FWD,
    ST_DIST_BWD,
    ST_MEDIAN_FWD,
    ST_MEDIAN_BWD,
    ST_FEAT_FWD,
    ST_FEAT_BWD,
    ST_FEAT_GATHER,
    ST_CONTRIB_WALK,
    ST_CONTRIB_GATHER,
    ST_COUNT
};
const char *kStageNames[ST_COUNT] = {"preprocess", "depth_sort", "instance_scan", "readback",
                                     "expand",     "tile_sort",  "tile_ranges",   "render_fwd",
                                     "render_bwd", "big_reduce", "preprocess_bwd", "sh_views",
                                     "bucket_count", "bucket_scatter", "seg_sort", "adam_sh_views",
                                     "background_grad", "distortion_fwd", "distortion_bwd",
                                     "median_fwd", "median_bwd",
                                     "feat_fwd", "feat_bwd", "feat_gather",
                                     "contrib_walk", "contrib_gather"};

struct Profiler {
    std::mutex mu;
    bool enabled = false;
    std::vector<hipEvent_t> pool;
    struct Pending {
        int stage;
        hipEvent_t a, b;
    };
    std::vector<Pending> pending;
    double total_ms[ST_COUNT] = {};
    int64_t calls[ST_COUNT] = {};

    hipEvent_t get() {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        return e;
    }
    void drain() {
        for (auto &p : pending) {
            float ms = 0.f;
            (void)hipEventSynchronize(p.b);
            if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
                total_ms[p.stage] += ms;
                calls[p.stage] += 1;
            }
            pool.push_back(p.a);
            pool.push_back(p.b);
        }
        pending.clear();
    }
};
Profiler &prof() {
    static Profiler p;
    return p;
}

// Scoped stage: records an event pair when profiling, synchronises + checks when debugging.
struct StageScope {
    hipStream_t s;
    int stage;
    bool debug;
    hipEvent_t a = nullptr;
    StageScope(hipStream_t s_, int st, bool dbg) : s(s_), stage(st), debug(dbg) {
        Profiler &p = prof();
        if (p.enabled && ((tuning(K_prof_mask) >> st) & 1)) {
            std::lock_guard<std::mutex> lk(p.mu);
            a = p.get();
            if (a) (void)hipEventRecord(a, s);
        }
    }
    int finish() {
        Profiler &p = prof();
        if (a) {
            std::lock_guard<std::mutex> lk(p.mu);
            hipEvent_t b = p.get();
            if (b) {
                (void)hipEventRecord(b, s);
                p.pending.push_back({stage, a, b});
            }
            if (p.pending.size() > 4096) p.drain();
        }
        hipError_t e = hipGetLastError();
        if (e == hipSuccess && debug) {
            e = hipStreamSynchronize(s);
            if (e == hipSuccess) e = hipGetLastError();
        }
        if (e != hipSuccess)
            return fail(GSR_ERR_HIP, std::string("stage ") + kStageNames[stage] + ": " + hipGetErrorString(e));
        return GSR_OK;
    }
};

#define GSR_STAGE(stage, dbg, ...)                      \
    do {                                                \
        StageScope sc_(stream, stage, dbg);             \
        __VA_ARGS__;                                    \
        int rc_ = sc_.finish();                         \
        if (rc_ != GSR_OK) return rc_;                  \
    } while (0)

// Every entry point runs with the device of its stream current (the caller's current device may differ, e.g. a
// thread rendering on cuda:1 after cuda:0), so scratch events, pinned words and launches all belong to the
// stream's device.  The null stream means the current device.
struct StreamDeviceGuard {
    int prev = -1, dev = -1;
    explicit StreamDeviceGuard(hipStream_t s) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        dev = prev;
        if (s && hipStreamGetDevice(s, &dev) != hipSuccess) dev = prev;
        if (dev != prev && dev >= 0) (void)hipSetDevice(dev);
        (void)hipGetLastError();
    }
    ~StreamDeviceGuard() {
        if (prev >= 0 && dev != prev) (void)hipSetDevice(prev);
    }
};

constexpr int kMaxDevices = 64;

// The readback event and pinned words are per thread AND per device: an event recorded on a stream of
// another device is an invalid handle.  One holder per thread owns them and releases them when the thread exits.
struct ReadbackSlots {
    hipEvent_t ev[64] = {};
    uint32_t *words[64] = {};
    ~ReadbackSlots() {
        for (int d = 0; d < 64; d++) {
            if (!ev[d] && !words[d]) continue;
            int prev = -1;
            if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(d) != hipSuccess) continue;
            if (ev[d]) (void)hipEventDestroy(ev[d]);
            if (words[d]) (void)hipHostFree(words[d]);
            if (prev >= 0) (void)hipSetDevice(prev);
        }
    }
};
ReadbackSlots &readback_slots() {
    thread_local ReadbackSlots s;
    return s;
}

hipEvent_t readback_event(int dev) {
    if (dev < 0 || dev >= kMaxDevices) return nullptr;
    hipEvent_t &e = readback_slots().ev[dev];
    if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
    return e;
}

// Instance total of the last forward on this thread and device (the binning buffer's pre-wait size hint).
int64_t &readback_hint(int dev) {
    thread_local int64_t h[kMaxDevices] = {};
    static int64_t none = 0;
    if (dev < 0 || dev >= kMaxDevices) return none = 0;
    return h[dev];
}

// Sequence number of the next preprocess readback on this thread and device (never 0: the buffer starts zeroed).
uint32_t next_readback_seq(int dev) {
    thread_local uint32_t seq[kMaxDevices] = {};
    if (dev < 0 || dev >= kMaxDevices) return 1u;
    if (++seq[dev] == 0u) seq[dev] = 1u;
    return seq[dev];
}

// Spin until the preprocess's last workgroup has published {total lo, hi, big count, seq} at hw[CNT_WORDS] (one
// 16-B store, read here with one 16-B load: aligned 16-B SSE loads are single-copy atomic on AVX-capable x86).
// Once the wait has lasted a millisecond the stream is queried every millisecond, so a failed launch or a kernel
// fault returns an error instead of spinning forever.  Not sooner: a hipStreamQuery puts a marker on the stream,
// and the next kernel's dispatch waited ~6 us behind it (a gap before the bucket scatter on every forward).
int wait_readback(const uint32_t *hw, uint32_t seq, hipStream_t s, uint64_t *total, uint32_t *nbig, uint32_t *kmin,
                  uint32_t *kmax) {
    const __m128i *src = reinterpret_cast<const __m128i *>(hw + CNT_WORDS);
    auto next_query = std::chrono::steady_clock::now() + std::chrono::milliseconds(1);
    for (uint64_t it = 1;; it++) {
        // the compiler barrier forces a fresh load every iteration (the GPU writes this memory behind the
        // compiler's back); a matching sequence word is accepted only when a second 16-B load returns the same
        // bytes, so even a torn read of the 16-B store could not hand back a stale total
        asm volatile("" ::: "memory");
        const __m128i v = _mm_load_si128(src);
        alignas(16) uint32_t w[4];
        _mm_store_si128(reinterpret_cast<__m128i *>(w), v);
        if (w[3] == seq) {
            asm volatile("" ::: "memory");
            const __m128i v2 = _mm_load_si128(src);
            if (_mm_movemask_epi8(_mm_cmpeq_epi8(v, v2)) != 0xffff) continue;
            *total = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
            *nbig = w[2];
            // the depth range word, stored just before (the same thread's earlier store; checked anyway)
            const __m128i *src2 = src + 1;
            for (uint64_t it2 = 0;; it2++) {
                asm volatile("" ::: "memory");
                const __m128i r = _mm_load_si128(src2);
                alignas(16) uint32_t q[4];
                _mm_store_si128(reinterpret_cast<__m128i *>(q), r);
                asm volatile("" ::: "memory");
                const __m128i r2 = _mm_load_si128(src2);
                if (q[2] == seq && _mm_movemask_epi8(_mm_cmpeq_epi8(r, r2)) == 0xffff) {
                    *kmin = q[0];
                    *kmax = q[1];
                    return GSR_OK;
                }
                if (it2 > (1u << 24)) return fail(GSR_ERR_HIP, "preprocess published its total without its depth range");
                _mm_pause();
            }
        }
        if ((it & 255) == 0 && std::chrono::steady_clock::now() >= next_query) {
            const hipError_t e = hipStreamQuery(s);
            if (e != hipSuccess && e != hipErrorNotReady) return fail(GSR_ERR_HIP, hipGetErrorString(e));
            if (e == hipSuccess && __atomic_load_n(hw + CNT_WORDS + 3, __ATOMIC_ACQUIRE) != seq)
                return fail(GSR_ERR_HIP, "preprocess finished without publishing its counters");
            next_query = std::chrono::steady_clock::now() + std::chrono::milliseconds(1);
        }
        _mm_pause();
    }
}

uint32_t *pinned_words(int dev) {
    if (dev < 0 || dev >= kMaxDevices) return nullptr;
    uint32_t *&p = readback_slots().words[dev];
    if (!p) {
        // coherent (fine-grained) pinned memory: the preprocess writes the counters here directly
        if (hipHostMalloc((void **)&p, 4096, hipHostMallocCoherent) != hipSuccess) p = nullptr;
        else memset(p, 0, 4096);
    }
    return p;
}

// Armed while a preprocess that publishes into this thread's pinned words may still be in flight: an early error
// return then waits for the stream, so the late store of an abandoned sequence number can never land after the
// next forward's (possibly on another stream) and hide it.
struct InflightReadback {
    hipStream_t s = nullptr;
    bool armed = false;
    ~InflightReadback() {
        if (armed) (void)hipStreamSynchronize(s);
    }
};

// The decoupled look-backs (instance scan, bucket tile scan, onesweep sorts) never wait on a predecessor that is not
// running: after lb_patience polls they recompute its aggregate from their input (wave_lookback's decoupled
// fallback), so every forward completes with exact output whatever the scheduling; the flags they leave (bit 2 of
// the counters' overflow word, bit 2 of a onesweep error word) only record that a fallback ran.  What remains to
// check is the instance scan's overflow bit (bit 0), which the debug forward reads back (the readback total already
// bounds the count, so this is a second line).  Onesweep error words exist only for the sorts that ran onesweep.
// Debug mode: the instance scan's overflow flag, and whether a decoupled look-back had to recompute a stalled
// predecessor (bit 2 of the counters' flag word and of the radix sorts' error words: exact either way, but a sign of
// a scheduling problem; reported to stderr).  sort_err: the radix sorts' error words that this forward cleared (the
// depth and the tile sort), or null.
int check_lookback_flags(hipStream_t s, int dev, const uint32_t *counters, const uint32_t *depth_err,
                         const uint32_t *tile_err) {
    uint32_t *hw = pinned_words(dev);
    if (!hw) return fail(GSR_ERR_HIP, "pinned host buffer allocation failed");
    hw[1] = hw[2] = 0u;
    GSR_HIP(hipMemcpyAsync(hw, counters + CNT_OVERFLOW, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (depth_err) GSR_HIP(hipMemcpyAsync(hw + 1, depth_err, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (tile_err) GSR_HIP(hipMemcpyAsync(hw + 2, tile_err, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    GSR_HIP(hipStreamSynchronize(s));
    if (hw[0] & 1u) return fail(GSR_ERR_OVERFLOW, "instance scan overflow");
    if ((hw[0] | hw[1] | hw[2]) & 4u)
        fprintf(stderr, "gsrast debug: a decoupled look-back recomputed a stalled predecessor\n");
    return GSR_OK;
}

int check_common(int P, int D, int M, int W, int H, const float *means3D, const float *opac,
                 const float *colors, const float *shs, const float *scales, const float *rots, const float *cov,
                 const float *view, const float *proj, const float *campos, const float *bg) {
    if (P < 0) return fail(GSR_ERR_ARG, "P must be >= 0");
    if (W <= 0 || H <= 0) return fail(GSR_ERR_ARG, "image_width and image_height must be positive");
    if ((int64_t)W * H > 0x7fffffffLL) return fail(GSR_ERR_ARG, "image too large");
    if ((uint64_t)P > (uint64_t)SCAN_TILE * SCAN_MAX_BLOCKS - 1)
        return fail(GSR_ERR_ARG, "too many Gaussians for the single-level scan");
    if (P == 0) return GSR_OK;
    if (!means3D || !opac) return fail(GSR_ERR_ARG, "means3D and opacities are required");
    if (!view || !proj || !bg) return fail(GSR_ERR_ARG, "viewmatrix, projmatrix and bg are required");
    if (!colors) {
        if (!shs || M <= 0) return fail(GSR_ERR_ARG, "Please provide exactly one of either SHs or precomputed colors!");
        if (D < 0 || D > 3) return fail(GSR_ERR_ARG, "sh_degree must be in [0, 3]");
        if ((D + 1) * (D + 1) > M) return fail(GSR_ERR_ARG, "sh_degree needs (deg+1)^2 coefficients per Gaussian");
        if (!campos) return fail(GSR_ERR_ARG, "campos is required with SHs");
    }
    if (!cov && (!scales || !rots))
        return fail(GSR_ERR_ARG, "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
    return GSR_OK;
}

// A caller's versioned struct (first member struct_size; fields are only ever appended) as the library reads it: the
// caller's min(struct_size, sizeof(T)) bytes over zeros.  A member the caller covers only in part is not there (get: 0).
template <typename T>
struct VersionedIn {
    T full{};
    size_t size;
    explicit VersionedIn(const T *x) : size(x->struct_size) { memcpy(&full, x, std::min(size, sizeof(T))); }
    template <typename M>
    bool covers(M T::*m) const {
        return (size_t)(reinterpret_cast<const char *>(&(full.*m)) - reinterpret_cast<const char *>(&full)) + sizeof(M) <= size;
    }
    template <typename M>
    M get(M T::*m) const { return covers(m) ? full.*m : M{}; }
};

// gsr_composite_ext as the library reads it (all NULL without the struct: gsr_forward / gsr_backward)
struct CompositeExt {
    bool given = false;
    const float *background_image = nullptr;
    float *out_alpha = nullptr;
    const float *dL_dalpha = nullptr;
    float *dL_dbackground = nullptr, *dL_dbackground_image = nullptr;
};
int read_composite_ext(const gsr_composite_ext *ext, const float *background, CompositeExt &e) {
    if (!ext) return GSR_OK;
    const VersionedIn<gsr_composite_ext> in(ext);
    if (!in.covers(&gsr_composite_ext::background_image))
        return fail(GSR_ERR_ARG, "gsr_composite_ext: struct_size ends before the first pointer field");
    e.given = true;
    e.background_image = in.get(&gsr_composite_ext::background_image);
    e.out_alpha = in.get(&gsr_composite_ext::out_alpha);
    e.dL_dalpha = in.get(&gsr_composite_ext::dL_dalpha);
    e.dL_dbackground = in.get(&gsr_composite_ext::dL_dbackground);
    e.dL_dbackground_image = in.get(&gsr_composite_ext::dL_dbackground_image);
    if (!background && !e.background_image)
        return fail(GSR_ERR_ARG, "one of background and gsr_composite_ext.background_image is required");
    return GSR_OK;
}

// gsr_absgrad_ext as the library reads it
struct AbsgradExt {
    float *dL_dmeans2D_abs = nullptr;
    int densify_abs = 0;
};
void read_absgrad_ext(const gsr_absgrad_ext *x, AbsgradExt &e) {
    if (!x) return;
    const VersionedIn<gsr_absgrad_ext> in(x);
    e.dL_dmeans2D_abs = in.get(&gsr_absgrad_ext::dL_dmeans2D_abs);
    e.densify_abs = in.get(&gsr_absgrad_ext::densify_abs);
}

// gsr_features_ext as the library reads it
struct FeaturesExt {
    bool given = false;
    int C = 0;
    const float *features = nullptr;
    float *out_features = nullptr;
    const float *dL_dout_features = nullptr;
    float *dL_dfeatures = nullptr;
};
// the checks both directions share: the struct's size, C and the features pointer
int read_features_ext(const gsr_features_ext *x, int P, FeaturesExt &f) {
    if (!x) return GSR_OK;
    const VersionedIn<gsr_features_ext> in(x);
    if (!in.covers(&gsr_features_ext::features))
        return fail(GSR_ERR_ARG, "gsr_features_ext: struct_size ends before the first pointer field");
    f.given = true;
    f.C = in.get(&gsr_features_ext::C);
    f.features = in.get(&gsr_features_ext::features);
    f.out_features = in.get(&gsr_features_ext::out_features);
    f.dL_dout_features = in.get(&gsr_features_ext::dL_dout_features);
    f.dL_dfeatures = in.get(&gsr_features_ext::dL_dfeatures);
    if (f.C < 1 || f.C > FEAT_MAX_C) return fail(GSR_ERR_ARG, "gsr_features_ext: C must be in [1, 64]");
    if (P > 0 && !f.features) return fail(GSR_ERR_ARG, "gsr_features_ext: features is required");
    return GSR_OK;
}

// gsr_distortion_ext as the library reads it
struct DistortionExt {
    bool given = false;
    int map = 0;
    float nearp = 0.f, farp = 0.f;
    float *out = nullptr, *tot_w = nullptr, *tot_m = nullptr;
    const float *dL_dD = nullptr;
};
// the checks both directions share: the struct's size, the map and its planes, the two totals
int read_distortion_ext(const gsr_distortion_ext *x, DistortionExt &d) {
    if (!x) return GSR_OK;
    const VersionedIn<gsr_distortion_ext> in(x);
    if (!in.covers(&gsr_distortion_ext::out_distortion))
        return fail(GSR_ERR_ARG, "gsr_distortion_ext: struct_size ends before the first pointer field");
    d.given = true;
    d.map = in.get(&gsr_distortion_ext::map);
    d.nearp = in.get(&gsr_distortion_ext::near_plane);
    d.farp = in.get(&gsr_distortion_ext::far_plane);
    d.out = in.get(&gsr_distortion_ext::out_distortion);
    d.tot_w = in.get(&gsr_distortion_ext::total_weight);
    d.tot_m = in.get(&gsr_distortion_ext::total_moment);
    d.dL_dD = in.get(&gsr_distortion_ext::dL_ddistortion);
    if (d.map != GSR_DISTORTION_Z && d.map != GSR_DISTORTION_NDC)
        return fail(GSR_ERR_ARG, "gsr_distortion_ext: map must be GSR_DISTORTION_Z or GSR_DISTORTION_NDC");
    if (d.map == GSR_DISTORTION_NDC && !(d.nearp > 0.f && d.farp > d.nearp && std::isfinite(d.farp)))
        return fail(GSR_ERR_ARG, "gsr_distortion_ext: GSR_DISTORTION_NDC needs 0 < near_plane < far_plane");
    if (!d.tot_w || !d.tot_m)
        return fail(GSR_ERR_ARG, "gsr_distortion_ext: total_weight and total_moment are required");
    return GSR_OK;
}
// gsr_median_ext as the library reads it
struct MedianExt {
    bool given = false;
    float *out_depth = nullptr;
    int32_t *out_index = nullptr, *pos = nullptr;
    const float *dL_dmedian = nullptr;
};
// the checks both directions share: the struct's size and the position plane
int read_median_ext(const gsr_median_ext *x, MedianExt &m) {
    if (!x) return GSR_OK;
    const VersionedIn<gsr_median_ext> in(x);
    if (!in.covers(&gsr_median_ext::out_median_depth))
        return fail(GSR_ERR_ARG, "gsr_median_ext: struct_size ends before the first pointer field");
    m.given = true;
    m.out_depth = in.get(&gsr_median_ext::out_median_depth);
    m.out_index = in.get(&gsr_median_ext::out_median_index);
    m.pos = in.get(&gsr_median_ext::median_pos);
    m.dL_dmedian = in.get(&gsr_median_ext::dL_dmedian_depth);
    if (!m.pos) return fail(GSR_ERR_ARG, "gsr_median_ext: median_pos is required");
    return GSR_OK;
}
// far / (far - near) and far near / (far - near), formed in double and rounded once
static float dist_k0(const DistortionExt &d) { return (float)((double)d.farp / ((double)d.farp - (double)d.nearp)); }
static float dist_dscale(const DistortionExt &d) {
    return (float)((double)d.farp * (double)d.nearp / ((double)d.farp - (double)d.nearp));
}

}  // namespace

extern "C" {

size_t gsr_geom_buffer_bytes(int P) {
    GeomState g;
    return carve_geom(nullptr, P, g);
}
size_t gsr_binning_buffer_bytes(int64_t R, int W, int H) {
    BinningState b;
    uint32_t T = (uint32_t)(((W + BLOCK_X - 1) / BLOCK_X) * ((H + BLOCK_Y - 1) / BLOCK_Y));
    return carve_binning(nullptr, R, T, b);
}
size_t gsr_image_buffer_bytes(int W, int H) {
    ImageState im;
    return carve_image(nullptr, W, H, im);
}
static size_t bwd_scratch_size(int64_t R, int64_t nbig, bool abs, int feat_block) {
    BwdScratch sc;
    return carve_bwd_scratch(nullptr, R, nbig, abs, feat_block, sc);
}
size_t gsr_bwd_scratch_bytes(int64_t R, int64_t num_big) { return bwd_scratch_size(R, num_big, false, 0); }
size_t gsr_bwd_scratch_bytes_abs(int64_t R, int64_t num_big) { return bwd_scratch_size(R, num_big, true, 0); }
size_t gsr_bwd_scratch_bytes_features(int64_t R, int64_t num_big, int C) {
    return (C < 1 || C > FEAT_MAX_C) ? 0 : bwd_scratch_size(R, num_big, false, feat_block(C));
}

// gsr_contributions' scratch: one 16-B row per instance, then one per big Gaussian (num_big < 0: the most there can
// be, as the backward sizes its sums).  A null base returns the size only.
static size_t carve_contrib_scratch(char *base, int64_t R, int64_t num_big, uint4 **rows, uint4 **bigsum) {
    if (R < 0) R = 0;
    const int64_t nbig = num_big < 0 ? R / (BIG_GAUSSIAN_TILES + 1) + 1 : num_big;
    Carver c(base);
    uint4 *r = c.take<uint4>((size_t)(R ? R : 1));
    uint4 *b = c.take<uint4>((size_t)(nbig ? nbig : 1));
    if (rows) *rows = r;
    if (bigsum) *bigsum = b;
    return align_up(c.off, 256);
}
size_t gsr_contrib_scratch_bytes(int64_t R, int64_t num_big) {
    return carve_contrib_scratch(nullptr, R, num_big, nullptr, nullptr);
}

void gsr_state_layout_query(int P, int64_t R, int W, int H, gsr_state_layout *caller) {
    if (!caller) return;
    // versioned: fill a full struct here, copy back only the caller's size (fields are only appended)
    const size_t want = caller->struct_size ? std::min(caller->struct_size, sizeof(gsr_state_layout))
                                            : sizeof(gsr_state_layout);
    gsr_state_layout full{};
    gsr_state_layout *out = &full;
    char *const base = reinterpret_cast<char *>(size_t(1) << 40);  // any aligned non-null base
    auto off = [&](const void *p) { return (size_t)(reinterpret_cast<const char *>(p) - base); };
    GeomState g;
    carve_geom(base, P, g);
    BinningState b;
    const uint32_t T = (uint32_t)(((W + BLOCK_X - 1) / BLOCK_X) * ((H + BLOCK_Y - 1) / BLOCK_Y));
    carve_binning(base, R, T, b);
    ImageState im;
    carve_image(base, W, H, im);
    out->geom_rec_a = off(&g.rec->a);
    out->geom_rec_b = off(&g.rec->b);
    out->geom_rec_c = off(&g.rec->c);
    out->geom_rec_stride = sizeof(GRec);
    out->geom_tiles = off(g.tiles);
    out->geom_order = off(g.order);
    out->geom_inst_off = off(g.inst_off);
    out->geom_inst_start = off(g.inst_start);
    out->geom_clamped = off(g.clamped);
    out->geom_expand_rec = off(g.exp_rec);
    out->geom_depth_key = off(g.depth_key);
    out->bin_point_list = off(b.point_list);
    out->bin_inv = off(b.inv);
    out->bin_keys_sorted = off(b.keys_sorted);
    out->bin_sorted_u = off(b.sorted_u);
    out->bin_inst_gid = off(b.inst_gid);
    out->img_tile_loaded = off(im.tile_loaded);
    out->bin_bk_keys = off(b.bk_keys);
    out->img_final_T = off(im.final_T);
    out->img_n_contrib = off(im.n_contrib);
    out->img_ranges = off(im.ranges);
    out->img_tile_last = off(im.tile_last);
    full.struct_size = want;
    memcpy(caller, &full, want);
}

// The state a forward call builds in its three buffers, as the forward fills it and as the backward and
// gsr_contributions recover it from the caller's buffers (recover_state)
struct RasterState {
    int W, H, gx, gy;
    uint32_t T, R;
    // recover_state with num_big < 0: not known on the host (the upstream backward signature has no such argument,
    // gsr_torch_ext): nbig is then the most there can be (each has > BIG_GAUSSIAN_TILES instances), which sizes the
    // sums, and nbig_dev the count the preprocess left in the geometry buffer, which the reductions read; else nbig is
    // exact, nbig_dev null
    uint32_t nbig;
    const uint32_t *nbig_dev;
    GeomState g;
    BinningState b;
    ImageState im;
};
static void set_image(RasterState &s, int W, int H) {
    s.W = W, s.H = H;
    s.gx = (W + BLOCK_X - 1) / BLOCK_X, s.gy = (H + BLOCK_Y - 1) / BLOCK_Y;
    s.T = (uint32_t)(s.gx * s.gy);
}
static void recover_state(RasterState &s, int P, int W, int H, int64_t R, int64_t num_big, const void *geom,
                          const void *binning, const void *image) {
    set_image(s, W, H);
    s.R = (uint32_t)R;
    carve_geom(static_cast<char *>(const_cast<void *>(geom)), P, s.g);
    carve_binning(static_cast<char *>(const_cast<void *>(binning)), s.R, s.T, s.b);
    carve_image(static_cast<char *>(const_cast<void *>(image)), W, H, s.im);
    s.nbig = num_big < 0 ? s.R / (BIG_GAUSSIAN_TILES + 1) + 1 : (uint32_t)num_big;
    s.nbig_dev = num_big < 0 ? s.g.counters + CNT_BIG : nullptr;
}
// What the gathers test (gsr_gather.h).  live: the backward composite's flags apply ("bwd_live" 1); the validity word
// goes with every backward, as it always did, and is null only where no backward composite ran (gsr_contributions)
static GatherSrc gather_src(const int *radii, const RasterState &s, bool backward, bool live) {
    GatherSrc src;
    src.radii = radii; src.tiles = s.g.tiles; src.inst_start = s.g.inst_start;
    src.big_slot = s.g.big_slot; src.big_list = s.g.big_list; src.inv = s.b.inv;
    src.live = backward && live ? s.g.live : nullptr;
    src.live_valid = backward ? s.g.counters + CNT_LIVE_VALID : nullptr;
    return src;
}
// What the replays read (gsr_replay.h)
static ReplaySrc replay_src(const RasterState &s) {
    ReplaySrc r;
    r.W = s.W; r.H = s.H; r.gx = s.gx; r.gy = s.gy; r.num_tiles = (int)s.T;
    r.ranges = s.im.ranges; r.point_list = s.b.point_list; r.n_contrib = s.im.n_contrib;
    r.tile_last = s.im.tile_last; r.tile_loaded = s.im.tile_loaded; r.sorted_u = s.b.sorted_u;
    r.rec = s.g.rec;
    return r;
}

// One forward call's state: what the argument checks read, the state it builds, and what one stage leaves for the
// next.  Each stage below takes it whole, in the driver's order (gsr_forward_features).
struct FwdCall : RasterState {
    gsr_forward_args *a;
    gsr_alloc_fn alloc;
    void *alloc_ctx;
    hipStream_t stream;
    bool dbg;
    int dev;  // the stream's device (StreamDeviceGuard)
    CompositeExt e;
    FeaturesExt fx;
    DistortionExt dx;
    MedianExt mx;
    int P;
    // the readback: this thread's pinned words and event, the sequence number awaited, and whether the preprocess
    // publishes into the words ("rb_spin") or a copy plus the event brings the counters
    uint32_t *hw;
    hipEvent_t rb_ev;
    uint32_t seq;
    bool rb_spin;
    InflightReadback *inflight;  // the driver's
    int bk, lpt;                 // the "bucket" and "lpt" knobs
    bool bk_possible;            // the tile count admits the bucket path: its count pass is queued
    BucketParams bp;
    char *bin;                   // the binning buffer requested before the wait (bin_cap instances), or null
    int64_t bin_cap;
    uint32_t kmin, kmax;         // the kept depth keys' range (kmin > kmax: none kept)
    bool bucket;                 // bucket binning, else the radix path
    bool xcd_fwd;                // the composite runs the per-XCD LPT orders (set by the bucket scatter)
};

// The side structs and every argument check, in the order callers see their errors
static int fwd_check_args(FwdCall &c, const gsr_composite_ext *ext, const gsr_features_ext *feat,
                          const gsr_distortion_ext *dist, const gsr_median_ext *median) {
    gsr_forward_args *a = c.a;
    int rc = read_composite_ext(ext, a->background, c.e);
    if (rc) return rc;
    rc = read_features_ext(feat, a->P, c.fx);
    if (rc) return rc;
    if (c.fx.given && !c.fx.out_features) return fail(GSR_ERR_ARG, "gsr_features_ext: out_features is required");
    rc = read_distortion_ext(dist, c.dx);
    if (rc) return rc;
    if (c.dx.given && !c.dx.out) return fail(GSR_ERR_ARG, "gsr_distortion_ext: out_distortion is required");
    rc = read_median_ext(median, c.mx);
    if (rc) return rc;
    if (c.mx.given && (!c.mx.out_depth || !c.mx.out_index))
        return fail(GSR_ERR_ARG, "gsr_median_ext: out_median_depth and out_median_index are required");
    rc = check_common(a->P, a->D, a->M, a->W, a->H, a->means3D, a->opacities, a->colors_precomp, a->shs,
                      a->scales, a->rotations, a->cov3D_precomp, a->viewmatrix, a->projmatrix, a->campos,
                      c.e.background_image ? c.e.background_image : a->background);
    if (rc) return rc;
    if (!a->out_color || (a->P > 0 && !a->radii)) return fail(GSR_ERR_ARG, "out_color and radii are required");
    c.P = a->P;
    set_image(c, a->W, a->H);
    return GSR_OK;
}

// P == 0: the reference returns its zero-initialised outputs untouched; with a gsr_composite_ext the colour is what
// the composite writes where no Gaussian reaches: the background, alpha 0
static int fwd_empty_scene(FwdCall &c) {
    gsr_forward_args *a = c.a;
    hipStream_t stream = c.stream;
    const size_t HW = (size_t)c.W * c.H;
    if (c.e.given) {
        launch_background_fill(stream, HW, a->background, c.e.background_image, a->out_color, c.e.out_alpha);
        GSR_HIP(hipGetLastError());
    } else {
        GSR_HIP(hipMemsetAsync(a->out_color, 0, sizeof(float) * 3 * HW, stream));
    }
    if (a->out_invdepth) GSR_HIP(hipMemsetAsync(a->out_invdepth, 0, sizeof(float) * HW, stream));
    if (c.fx.given) GSR_HIP(hipMemsetAsync(c.fx.out_features, 0, sizeof(float) * c.fx.C * HW, stream));
    if (c.dx.given)
        for (float *m : {c.dx.out, c.dx.tot_w, c.dx.tot_m}) GSR_HIP(hipMemsetAsync(m, 0, sizeof(float) * HW, stream));
    if (c.mx.given) {  // no Gaussian reaches any pixel: depth 0, index and position -1
        GSR_HIP(hipMemsetAsync(c.mx.out_depth, 0, sizeof(float) * HW, stream));
        GSR_HIP(hipMemsetAsync(c.mx.out_index, 0xff, sizeof(int32_t) * HW, stream));
        GSR_HIP(hipMemsetAsync(c.mx.pos, 0xff, sizeof(int32_t) * HW, stream));
    }
    return GSR_OK;
}

// The bucket path's parameters as far as they are known before the instance total (its count pass), the walk block
// count included
static int fwd_bucket_plan(FwdCall &c) {
    const GeomState &g = c.g;
    const ImageState &im = c.im;
    const int P = c.P;
    BucketParams &bp = c.bp;
    bp.P = (uint32_t)P; bp.T = c.T; bp.gx = c.gx; bp.nbig = g.counters + CNT_BIG;
    bp.nb = std::max(1u, std::min({256u, BK_MAX_BLOCKS, div_up(P, 1024)}));  // 192 / 384 walk blocks measured slower (A.2)
    bp.gper = div_up(div_up(P, bp.nb), 256) * 256;  // whole preprocess blocks
    bp.nr = div_up(P, bp.gper);
    // extra walk blocks for the big rects (used only when the device's big-Gaussian count exceeds nr: bk_walk_blocks);
    // the block count is fixed here, before that count is read back.  2000 sparse-scene Gaussians at 1080p ran their
    // big rects on 2 blocks (count + scatter walks 220 + 310 us).  Only below half of that count of
    // range blocks: at cfg 3 (245 range blocks) 11 extra blocks measured +10 us of scatter (profiles/r4s_*)
    const uint32_t big_blocks = std::min((uint32_t)tuning(K_bk_big_blocks), BK_MAX_BLOCKS);
    bp.nb = 2 * bp.nr < big_blocks ? big_blocks : bp.nr;
    bp.tiles = g.tiles; bp.inst_start = g.inst_start; bp.block_sums = g.block_sums; bp.depth_key = g.depth_key;
    bp.big_list = g.big_list; bp.exp_rec = g.exp_rec;
    bp.hist = im.bk_hist; bp.hist_pre = im.bk_hist_pre; bp.tile_next = im.bk_tile_next; bp.reg_start = im.bk_reg_start;
    bp.tile_start = im.bk_tile_start; bp.ranges = im.ranges;
    bp.tile_last = im.tile_last; bp.tile_loaded = im.tile_loaded;
    bp.lpt_bcnt = im.lpt_bcnt;
    bp.ticket = g.counters + CNT_COL_TICKET; bp.tile_status = g.tile_status; bp.err = g.counters + CNT_OVERFLOW;
    bp.long_list = im.bk_long_list; bp.long_cnt = g.counters + CNT_LONG;
    bp.lb_patience = LB_PATIENCE; bp.lb_force = tuning(K_lb_force);
    bp.xcd_major = tuning(K_bk_xcd);
    // every buffer the column pass clears must be wired (a null one would fault the GPU, not fail here)
    if (!bp.tile_last || !bp.tile_loaded || !bp.ranges || !bp.tile_start || !bp.hist_pre)
        return fail(GSR_ERR_ARG, "internal: bucket binning buffer not set");
    return GSR_OK;
}

// The geometry and image buffers, the counter clear, the preprocess and -- queued right behind it, before the host
// waits for the total -- the bucket path's count pass
static int fwd_preprocess(FwdCall &c) {
    gsr_forward_args *a = c.a;
    hipStream_t stream = c.stream;
    const int P = c.P, W = c.W, H = c.H;
    GeomState &g = c.g;
    char *geom = c.alloc(c.alloc_ctx, GSR_BUF_GEOM, carve_geom(nullptr, P, g));
    if (!geom) return fail(GSR_ERR_ALLOC, "geometry buffer allocation failed");
    carve_geom(geom, P, g);
    char *img = c.alloc(c.alloc_ctx, GSR_BUF_IMAGE, carve_image(nullptr, W, H, c.im));
    if (!img) return fail(GSR_ERR_ALLOC, "image buffer allocation failed");
    carve_image(img, W, H, c.im);
    // counters + instance-scan and tile-scan look-back words; rounded up to the carver's 256-B alignment (the
    // next array starts there) so the memset is one aligned fill kernel, not an aligned fill plus a tail
    const size_t clear_bytes = align_up((size_t)(reinterpret_cast<char *>(g.tile_status + BK_MAX_TILES / 32 + 1) -
                                                 reinterpret_cast<char *>(g.counters)), 256);
    launch_zero16(stream, g.counters, clear_bytes);  // a plain kernel: the runtime's fill measured slower

    PreprocessParams pp;
    pp.P = P; pp.D = a->D; pp.M = a->M; pp.W = W; pp.H = H; pp.gx = c.gx; pp.gy = c.gy;
    pp.tan_fovx = a->tan_fovx; pp.tan_fovy = a->tan_fovy;
    pp.focal_x = W / (2.0f * a->tan_fovx);
    pp.focal_y = H / (2.0f * a->tan_fovy);
    pp.scale_modifier = a->scale_modifier;
    pp.antialiasing = a->antialiasing;
    pp.cull = tuning(K_cull);
    pp.means3D = a->means3D; pp.opacities = a->opacities; pp.scales = a->scales; pp.rotations = a->rotations;
    pp.cov3D_precomp = a->cov3D_precomp; pp.colors_precomp = a->colors_precomp; pp.shs = a->shs;
    pp.view = a->viewmatrix; pp.proj = a->projmatrix; pp.campos = a->campos;
    pp.radii = a->radii;
    pp.g = g;
    // The bucket path's Gaussian-order instance scan is formed by its count pass from these block totals.
    pp.block_sums = g.block_sums;
    // The instance total only needs the per-Gaussian tile counts, so it is read back right after the
    // preprocess: its last workgroup writes the counters into pinned host memory and then a sequence word the
    // host polls (debug = 1: a copy plus an event, one more kernel and a barrier on the stream).
    c.hw = pinned_words(c.dev);
    c.rb_ev = readback_event(c.dev);
    if (!c.hw || !c.rb_ev) return fail(GSR_ERR_HIP, "pinned host buffer / event allocation failed");
    c.rb_spin = !c.dbg;
    c.seq = next_readback_seq(c.dev);
    pp.host_words = c.rb_spin ? c.hw : nullptr;
    pp.stamps = tuning(K_stamp) ? stamp_buffer(3) : nullptr;
    pp.seq = c.seq;
    // armed before the launch: an error reported after it, by this stage or a later one, still waits for the kernel
    // (the driver's frame holds it until the call returns)
    c.inflight->s = stream;
    c.inflight->armed = c.rb_spin;
    // the kept depth keys' range, for the radix path's relative depth sort: only where that sort can run (multi-kernel
    // depth sorts, P above the onesweep limit); else the range words stay empty and the sort takes its 32-bit keys
    pp.depth_range = (tuning(K_depth_rel) && (uint32_t)P > (uint32_t)tuning(K_onesweep_max_n)) ? 1 : 0;
    GSR_STAGE(ST_PREPROCESS, c.dbg, launch_preprocess(stream, pp));
    if (!c.rb_spin) {
        GSR_HIP(hipMemcpyAsync(c.hw, g.counters, CNT_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        GSR_HIP(hipEventRecord(c.rb_ev, stream));
    }
    // The bucket path's count pass needs no total either: whenever the tile count admits that path it is queued
    // right behind the preprocess, so the GPU runs it while the host waits (its scratch is in the image buffer;
    // if the total then selects the radix path, its results are simply unused).
    c.bk = tuning(K_bucket);
    c.bk_possible = c.bk == 2 ? c.T <= BK_MAX_TILES : c.bk == 1 && c.T <= BK_MAX_TILES / 2;
    c.lpt = tuning(K_lpt);
    if (c.bk_possible) {
        const int rc = fwd_bucket_plan(c);
        if (rc) return rc;
        GSR_STAGE(ST_BK_COUNT, c.dbg, launch_bucket_count(stream, c.bp));
    }
    return GSR_OK;
}

// The instance total and the big-Gaussian count, read back; which binning path the total selects
static int fwd_readback(FwdCall &c) {
    hipStream_t stream = c.stream;
    // The binning buffer's size depends on the instance total.  Requesting it through the caller's allocator
    // (a Python callback from rasterizer.py) after the readback put ~40 us of host work between the preprocess and
    // the next launch, longer than the queued count passes cover; so with a total from an earlier call on this
    // thread and device (readback_hint, read here before the wait) the buffer is requested before the wait, 25 %
    // larger, and only re-requested when the total exceeds it.
    c.bin = nullptr;
    c.bin_cap = -1;
    const int64_t r_hint = readback_hint(c.dev);
    if (r_hint > 0) {
        c.bin_cap = std::min<int64_t>(r_hint + r_hint / 4 + 4096, 0xffffffffLL);
        c.bin = c.alloc(c.alloc_ctx, GSR_BUF_BINNING, carve_binning(nullptr, c.bin_cap, c.T, c.b));
        if (!c.bin) return fail(GSR_ERR_ALLOC, "binning buffer allocation failed");
    }
    uint64_t total64 = 0;
    c.nbig = 0, c.kmin = 0xffffffffu, c.kmax = 0;
    if (c.rb_spin) {
        GSR_STAGE(ST_READBACK, c.dbg, {
            const int rc = wait_readback(c.hw, c.seq, stream, &total64, &c.nbig, &c.kmin, &c.kmax);
            if (rc) return rc;
        });
        c.inflight->armed = false;  // published: the pinned words are this call's no longer
    } else {
        GSR_STAGE(ST_READBACK, c.dbg, GSR_HIP(hipEventSynchronize(c.rb_ev)));
        uint32_t cmax = 0;
        for (int k = 0; k < CNT_NPART; k++) {
            uint64_t part;
            memcpy(&part, c.hw + CNT_PARTIALS + 2 * k, sizeof(part));
            total64 += part;
            cmax = std::max(cmax, c.hw[CNT_DMIN + k]);
            c.kmax = std::max(c.kmax, c.hw[CNT_DMAX + k]);
        }
        c.kmin = ~cmax;
        c.nbig = c.hw[CNT_BIG];
    }
    if (total64 > 0xffffffffull) return fail(GSR_ERR_OVERFLOW, "more than 2^32-1 tile instances");
    c.R = (uint32_t)total64;
    // Bucket binning (gsr_bin.hip) while the tile counters fit a workgroup's LDS with room for two per CU and
    // the tiles are short (per-tile sorts cost n log^2 n): at 1M Gaussians / 1080p (517 instances per tile) it
    // takes 0.20 ms against the radix path's 0.30; at 5M / 4K stress (1240 per tile) 4.4 ms against 1.4.
    // Otherwise the radix path: depth sort, depth-ordered expansion, stable tile sort.
    c.bucket = c.bk_possible && (c.bk == 2 || (uint64_t)c.R <= (uint64_t)BK_MAX_MEAN * c.T);
    if (c.bucket) g_stat_depth_passes.store(0, std::memory_order_relaxed);
    return GSR_OK;
}

// Radix path: the depth sort and the instance scan, launched before the binning buffer is sized so that the GPU
// runs them meanwhile
static int fwd_depth_sort(FwdCall &c) {
    hipStream_t stream = c.stream;
    GeomState &g = c.g;
    const int P = c.P;
    // the depth sort's last pass also writes the tile counts in depth order, so the instance scan reads them
    // coalesced instead of gathering them through the order (the expansion records it leaves to the expansion's gather
    // by rank: writing them too measured slower, cfg 5 depth sort 0.232 -> 0.352 ms for expand 0.241 -> 0.221 ms,
    // profiles/r6t_libab_sort_gather_cfg5.txt)
    SortGather ga;
    ga.src = g.tiles; ga.dst = g.tiles_sorted;
    // Relative depth keys where the sort takes the multi-kernel path: the kept keys span
    // kmax - kmin, so rs_rel_key maps them onto [0, span] and the culled ones onto span + 1, and the sort runs
    // ceil(bits / 9) passes instead of 4 (cfg 5: 26 bits, 3 passes of 9 bits)
    int rel_bits = 32;
    if (tuning(K_depth_rel) && c.kmin <= c.kmax && (uint32_t)P > (uint32_t)tuning(K_onesweep_max_n) &&
        c.kmax - c.kmin < 0xfffffffeu)
        rel_bits = 32 - __builtin_clz(c.kmax - c.kmin + 1);
    g_stat_depth_passes.store(rel_bits <= 27 ? (rel_bits + 8) / 9 : 4, std::memory_order_relaxed);
    if (rel_bits <= 27)
        GSR_STAGE(ST_DEPTH_SORT, c.dbg,
                  launch_depth_sort_rel(stream, g.sort, (uint32_t)P, g.depth_key, c.kmin, c.kmax - c.kmin + 1, rel_bits,
                                        &ga));
    else
        GSR_STAGE(ST_DEPTH_SORT, c.dbg, launch_radix_sort(stream, g.sort, (uint32_t)P, 32, false, g.depth_key, &ga));
    GSR_STAGE(ST_SCAN, c.dbg,
              launch_exclusive_scan_lookback(stream, g.tiles_sorted, nullptr, (uint32_t)P, g.inst_off, g.scan_status,
                                             g.counters + CNT_SCAN_TICKET, g.counters + CNT_OVERFLOW));
    return GSR_OK;
}

// The binning buffer for R instances: the one requested before the wait if it is large enough, else a new one.  The
// total becomes the next call's hint here, after the wait and on the success path only.
static int fwd_binning_buffer(FwdCall &c) {
    readback_hint(c.dev) = c.R;
    if (!c.bin || (int64_t)c.R > c.bin_cap) {
        c.bin = c.alloc(c.alloc_ctx, GSR_BUF_BINNING, carve_binning(nullptr, c.R, c.T, c.b));
        if (!c.bin) return fail(GSR_ERR_ALLOC, "binning buffer allocation failed");
    }
    carve_binning(c.bin, c.R, c.T, c.b);  // offsets from R: a larger buffer only has unused space at the end
    if ((uint64_t)RS_BINS * div_up(c.R ? c.R : 1, RS_TILE) + 1 > (uint64_t)SCAN_TILE * SCAN_MAX_BLOCKS)
        return fail(GSR_ERR_OVERFLOW, "too many tile instances for the single-level scan");
    return GSR_OK;
}

// Bucket binning: the scatter into the tile buckets (and the forward LPT orders), then the per-tile sorts
static int fwd_bin_bucket(FwdCall &c) {
    hipStream_t stream = c.stream;
    const GeomState &g = c.g;
    const BinningState &b = c.b;
    const ImageState &im = c.im;
    const uint32_t T = c.T, R = c.R;
    const int lpt = c.lpt;
    if (R == 0) {
        GSR_HIP(hipMemsetAsync(im.ranges, 0, sizeof(uint2) * T, stream));
        if (lpt) launch_tile_order(stream, im.ranges, nullptr, 0, (int)T, im.order_fwd, im.lpt_hist);
        return GSR_OK;
    }
    BucketParams &bp = c.bp;
    bp.keys = b.bk_keys; bp.inst_gid = b.inst_gid; bp.inv = b.inv; bp.R = R;
    // region scatter: keys into 16-tile regions first (long runs per block), then a partition pass into the tile
    // buckets (gsr_bin.hip bk_partition_kernel)
    const int bkr = tuning(K_bk_region);
    // (the tile-in-region rides in u's top bits: R <= 2^28; the automatic choice also wants >= 256 keys per region
    // on average, so that a partition chunk rarely spans more regions than its LDS bins cover)
    const uint32_t nreg = div_up(T, BK_REGION);
    bp.keys_reg = ((bkr == 2 || (bkr == 1 && T > 4096 && R >= 256u * nreg)) && R <= (1u << BK_REG_SHIFT))
                      ? b.bk_keys2 : nullptr;
    bp.order = lpt ? im.order_fwd : nullptr;
    // per-XCD LPT orders for the whole-tile composites (with the backward's bucket lists)
    c.xcd_fwd = lpt && lpt_append_range(T) && tuning(K_xcd_lpt) &&
                render_fwd_parts((int)T) == 1;
    bp.order_xcd = c.xcd_fwd ? im.order_xcd : nullptr;
    bp.lpt_shift = LPT_SHIFT;
    GSR_STAGE(ST_BK_SCATTER, c.dbg, launch_bucket_scatter(stream, bp));  // and the forward LPT order
    SegSortParams sp;
    sp.T = T; sp.ranges = im.ranges;
    sp.tile_order = lpt ? im.order_fwd : nullptr;  // the long tiles lead it (LPT_SHIFT)
    sp.keys = b.bk_keys; sp.keys2 = b.bk_keys2;
    sp.sorted_u = b.sorted_u; sp.long_list = im.bk_long_list; sp.long_cnt = g.counters + CNT_LONG;
    GSR_STAGE(ST_SEG_SORT, c.dbg, launch_seg_sort(stream, sp));
    return GSR_OK;
}

// Radix binning: the depth-ordered expansion, the stable tile sort and the tile ranges
static int fwd_bin_radix(FwdCall &c) {
    hipStream_t stream = c.stream;
    const GeomState &g = c.g;
    BinningState &b = c.b;
    const ImageState &im = c.im;
    const uint32_t T = c.T, R = c.R;
    bool keys16 = false;
    if (R > 0) {
        ExpandParams ep;
        ep.P = (uint32_t)c.P; ep.R = R; ep.gx = c.gx; ep.gy = c.gy;
        ep.order = g.order; ep.inst_off = g.inst_off; ep.tiles = g.tiles; ep.exp_rec = g.exp_rec;
        ep.exp_sorted = nullptr;  // the depth sort leaves the records in place: gathered by rank
        ep.exp_owner = b.exp_owner;
        // 16-bit tile keys up to 65536 tiles ("tile_key16" 0: 32-bit): the tile sort, the expansion's key stores and
        // the range search move 2 bytes per key instead of 4
        const TileSortPlan plan = tile_sort_plan(T);
        keys16 = plan.k16;
        ep.keys_out = keys16 ? nullptr : b.sort.k[0];
        ep.keys16_out = keys16 ? reinterpret_cast<uint16_t *>(b.sort.k[0]) : nullptr;
        ep.inst_gid = b.inst_gid; ep.inst_start = g.inst_start; ep.inv_none = b.inv;
        GSR_STAGE(ST_EXPAND, c.dbg, launch_expand(stream, ep));
        if (keys16)
            GSR_STAGE(ST_TILE_SORT, c.dbg,
                      launch_radix_sort16(stream, b.sort, R, plan.digit_bits, plan.passes, tile_key_bits(T)));
        else
            GSR_STAGE(ST_TILE_SORT, c.dbg, launch_radix_sort(stream, b.sort, R, tile_key_bits(T)));
    }
    GSR_STAGE(ST_RANGES, c.dbg, {
        GSR_HIP(hipMemsetAsync(im.ranges, 0, sizeof(uint2) * T, stream));
        if (keys16) launch_identify_ranges16(stream, reinterpret_cast<const uint16_t *>(b.keys_sorted), R, im.ranges);
        else launch_identify_ranges(stream, b.keys_sorted, R, im.ranges);
    });
    if (c.lpt) launch_tile_order(stream, im.ranges, nullptr, 0, (int)T, im.order_fwd, im.lpt_hist);
    return GSR_OK;
}

// The composite: colour, inverse depth, alpha, and the state the backward and the replays read
static int fwd_composite(FwdCall &c) {
    gsr_forward_args *a = c.a;
    hipStream_t stream = c.stream;
    const GeomState &g = c.g;
    const BinningState &b = c.b;
    const ImageState &im = c.im;
    const uint32_t T = c.T;
    const int lpt = c.lpt;
    // split heavy tiles combine tile_last / tile_loaded with atomicMax: start from zero (adjacent arrays; the
    // bucket path's column pass clears them)
    if (!c.bucket || c.R == 0)
        GSR_HIP(hipMemsetAsync(im.tile_last, 0,
                               (size_t)(reinterpret_cast<char *>(im.lpt_bcnt + LPT_BCNT_WORDS) -
                                        reinterpret_cast<char *>(im.tile_last)),
                               stream));
    RenderFwdParams rp;
    rp.W = c.W; rp.H = c.H; rp.gx = c.gx; rp.gy = c.gy; rp.num_tiles = (int)T;
    rp.tile_order = lpt ? (c.xcd_fwd ? im.order_xcd : im.order_fwd) : nullptr;
    rp.xcd = c.xcd_fwd ? 1 : 0;
    rp.ranges = im.ranges; rp.sorted_u = b.sorted_u; rp.inst_gid = b.inst_gid;
    rp.point_list = b.point_list; rp.tile_loaded = im.tile_loaded;
    rp.inv = b.inv;
    rp.rec = g.rec;
    rp.bg = a->background ? a->background : c.e.background_image;
    rp.bg_image = c.e.background_image; rp.out_alpha = c.e.out_alpha;
    rp.out_color = a->out_color; rp.out_invdepth = a->out_invdepth; rp.final_T = im.final_T;
    rp.n_contrib = im.n_contrib; rp.tile_last = im.tile_last;
    // checkpoints for the segmented backward (spacing seg_k instances: 32 or a multiple of 64) while the image
    // has few tiles; the forward records in ck_flag whether it wrote them, so the backward never reads stale ones
    rp.ck_flag = im.ck_flag;
    // the backward's LPT order from bucket lists the whole-tile waves append (no ordering launch in the backward)
    rp.lpt_valid = im.lpt_valid;
    rp.strip_mask = b.strip_mask; rp.smask_valid = im.smask_valid;
    if (lpt_append_range(T) && lpt) {
        rp.lpt_bcnt = im.lpt_bcnt; rp.lpt_blist = im.lpt_blist;
    }
    if (T <= SEG_MAX_TILES && tuning(K_bwd_seg)) {
        rp.ckpt = b.ckpt; rp.ctot = im.ctot;
        const int k = tuning(K_seg_k);
        rp.ck_k = k <= 32 ? 32u : (uint32_t)(k / 64) * 64u;
    }
    if (c.R > 0 && (!rp.point_list || !rp.inst_gid || !rp.sorted_u))
        return fail(GSR_ERR_ARG, "internal: composite buffer not set");
    GSR_STAGE(ST_RENDER_FWD, c.dbg, launch_render_fwd(stream, rp));
    return GSR_OK;
}

// The feature image, replayed from what the composite just recorded (tile_last = 0: zeros)
static int fwd_features(FwdCall &c) {
    hipStream_t stream = c.stream;
    FeatFwdParams fp;
    fp.src = replay_src(c);
    fp.C = c.fx.C; fp.features = c.fx.features; fp.out = c.fx.out_features;
    GSR_STAGE(ST_FEAT_FWD, c.dbg, launch_feat_fwd(stream, fp));
    return GSR_OK;
}

// The distortion map and its two totals, replayed likewise (tile_last = 0: zeros)
static int fwd_distortion(FwdCall &c) {
    hipStream_t stream = c.stream;
    DistFwdParams dp;
    dp.src = replay_src(c);
    dp.depth_key = c.g.depth_key;
    dp.map = c.dx.map; dp.k0 = dist_k0(c.dx); dp.nearp = c.dx.nearp;
    dp.out = c.dx.out; dp.tot_w = c.dx.tot_w; dp.tot_m = c.dx.tot_m;
    GSR_STAGE(ST_DIST_FWD, c.dbg, launch_dist_fwd(stream, dp));
    return GSR_OK;
}

// The median depth, index and position planes, replayed likewise (tile_last = 0: 0, -1, -1)
static int fwd_median(FwdCall &c) {
    hipStream_t stream = c.stream;
    MedianFwdParams mp;
    mp.src = replay_src(c);
    mp.depth_key = c.g.depth_key;
    mp.out_depth = c.mx.out_depth; mp.out_index = c.mx.out_index; mp.out_pos = c.mx.pos;
    GSR_STAGE(ST_MEDIAN_FWD, c.dbg, launch_median_fwd(stream, mp));
    return GSR_OK;
}

int gsr_forward(gsr_forward_args *a, gsr_alloc_fn alloc, void *alloc_ctx, void *stream_ptr,
                int64_t *num_rendered) {
    return gsr_forward_ext(a, nullptr, alloc, alloc_ctx, stream_ptr, num_rendered);
}

int gsr_forward_ext(gsr_forward_args *a, const gsr_composite_ext *ext, gsr_alloc_fn alloc, void *alloc_ctx,
                    void *stream_ptr, int64_t *num_rendered) {
    return gsr_forward_features(a, ext, nullptr, alloc, alloc_ctx, stream_ptr, num_rendered);
}

int gsr_forward_features(gsr_forward_args *a, const gsr_composite_ext *ext, const gsr_features_ext *feat,
                         gsr_alloc_fn alloc, void *alloc_ctx, void *stream_ptr, int64_t *num_rendered) {
    return gsr_forward_distortion(a, ext, feat, nullptr, alloc, alloc_ctx, stream_ptr, num_rendered);
}

int gsr_forward_distortion(gsr_forward_args *a, const gsr_composite_ext *ext, const gsr_features_ext *feat,
                           const gsr_distortion_ext *dist, gsr_alloc_fn alloc, void *alloc_ctx, void *stream_ptr,
                           int64_t *num_rendered) {
    return gsr_forward_median(a, ext, feat, dist, nullptr, alloc, alloc_ctx, stream_ptr, num_rendered);
}

int gsr_forward_median(gsr_forward_args *a, const gsr_composite_ext *ext, const gsr_features_ext *feat,
                       const gsr_distortion_ext *dist, const gsr_median_ext *median, gsr_alloc_fn alloc,
                       void *alloc_ctx, void *stream_ptr, int64_t *num_rendered) {
    if (!a || !alloc || !num_rendered) return fail(GSR_ERR_ARG, "null argument");
    FwdCall c{};
    c.a = a; c.alloc = alloc; c.alloc_ctx = alloc_ctx;
    c.stream = (hipStream_t)stream_ptr; c.dbg = a->debug != 0;
    int rc = fwd_check_args(c, ext, feat, dist, median);
    if (rc) return rc;
    // Both live in this frame across every stage: the stream's device stays current until the call returns, and an
    // early return of any stage after the preprocess launch runs ~InflightReadback (a wait for the stream) before
    // this thread's pinned words can be reused.  Destroyed in this order: the wait, then the device restored.
    StreamDeviceGuard device_guard(c.stream);
    InflightReadback inflight;
    c.dev = device_guard.dev;
    c.inflight = &inflight;
    *num_rendered = 0;
    a->num_big_out = 0;
    if (c.P == 0) return fwd_empty_scene(c);
    rc = fwd_preprocess(c);
    if (!rc) rc = fwd_readback(c);
    if (rc) return rc;
    *num_rendered = c.R;
    a->num_big_out = c.nbig;
    if (!c.bucket) rc = fwd_depth_sort(c);
    if (!rc) rc = fwd_binning_buffer(c);
    if (!rc) rc = c.bucket ? fwd_bin_bucket(c) : fwd_bin_radix(c);
    if (!rc) rc = fwd_composite(c);
    if (!rc && c.fx.given) rc = fwd_features(c);
    if (!rc && c.dx.given) rc = fwd_distortion(c);
    if (!rc && c.mx.given) rc = fwd_median(c);
    if (rc || !c.dbg) return rc;
    // every radix sort clears its error word (onesweep: with its control block; multi-kernel: pass 0)
    return check_lookback_flags(c.stream, c.dev, c.g.counters, c.bucket ? nullptr : c.g.sort.ctrl + RS_CTRL_ERR,
                                c.bucket || c.R == 0 ? nullptr : c.b.sort.ctrl + RS_CTRL_ERR);
}

// The per-Gaussian outputs preprocess_bwd writes for Gaussians [g0, g1), as zero-fill segments of the composite backward
// (RenderBwdParams::zf_*): each output's 16-B aligned interior, its unaligned head / tail words listed.  At cfg 3,
// 78 % of the Gaussians have an identically zero gradient (culled, or no pixel took one; tools/zero_grad_census.py):
// their ~250 B of zeros are stored by the VALU-bound walk instead of the HBM-bound per-Gaussian pass.  False (no
// plan): a pointer not 4-B aligned, or too many segments / odd words.
static bool zero_fill_plan(const gsr_backward_args *a, float *dL_dmeans2D_abs, int64_t g0, int64_t g1,
                           RenderBwdParams &rp) {
    const size_t ng = (size_t)(g1 - g0);
    const bool sh_stage = !a->colors_precomp && a->shs && a->M > 0;  // preprocess_bwd writes the SH outputs
    struct Out { float *p; size_t w; };
    const Out outs[] = {{a->dL_dmeans2D, 3}, {a->dL_dcolors, 3}, {a->dL_dopacity, 1}, {a->dL_dmeans3D, 3},
                        {a->dL_dcov3D, 6}, {sh_stage ? a->dL_dsh : nullptr, (size_t)a->M * 3},
                        {sh_stage ? a->dL_dcolors_sh : nullptr, 3}, {a->dL_dscales, 3}, {a->dL_drotations, 4},
                        {dL_dmeans2D_abs, 2}};
    static_assert(sizeof(outs) / sizeof(outs[0]) <= (size_t)RenderBwdParams::ZF_SEGS &&
                      6 * sizeof(outs) / sizeof(outs[0]) <= (size_t)RenderBwdParams::ZF_ODD,
                  "one segment and up to 3 + 3 odd words per output");
    RenderBwdParams z = rp;
    z.zf_nseg = z.zf_nodd = 0;
    z.zf_total16 = 0;
    for (const Out &o : outs) {
        if (!o.p || ng == 0) continue;
        const uintptr_t b = reinterpret_cast<uintptr_t>(o.p), e = b + ng * o.w * sizeof(float);
        if (b & 3) return false;
        const uintptr_t ab = std::min((b + 15) & ~(uintptr_t)15, e), ae = std::max(e & ~(uintptr_t)15, ab);
        for (uintptr_t q = b; q < ab; q += 4) {
            if (z.zf_nodd >= (uint32_t)RenderBwdParams::ZF_ODD) return false;
            z.zf_odd[z.zf_nodd++] = reinterpret_cast<uint32_t *>(q);
        }
        for (uintptr_t q = ae; q < e; q += 4) {
            if (z.zf_nodd >= (uint32_t)RenderBwdParams::ZF_ODD) return false;
            z.zf_odd[z.zf_nodd++] = reinterpret_cast<uint32_t *>(q);
        }
        if (ae > ab) {
            if (z.zf_nseg >= (uint32_t)RenderBwdParams::ZF_SEGS) return false;
            z.zf_ptr[z.zf_nseg] = reinterpret_cast<uint4 *>(ab);
            z.zf_total16 += (ae - ab) / 16;
            z.zf_pre16[++z.zf_nseg] = z.zf_total16;
        }
    }
    rp = z;
    return true;
}

// The camera gradients (dL_dviewmatrix / dL_dprojmatrix / dL_dcampos): written by the per-Gaussian stage
static bool camera_grads(const gsr_backward_args *a) {
    return a->stages != GSR_BWD_COMPOSITE && (a->dL_dviewmatrix || a->dL_dprojmatrix || a->dL_dcampos);
}
static int zero_camera_grads(const gsr_backward_args *a, hipStream_t stream) {  // no Gaussian: the empty sum
    if (a->dL_dviewmatrix) GSR_HIP(hipMemsetAsync(a->dL_dviewmatrix, 0, sizeof(float) * 16, stream));
    if (a->dL_dprojmatrix) GSR_HIP(hipMemsetAsync(a->dL_dprojmatrix, 0, sizeof(float) * 16, stream));
    if (a->dL_dcampos) GSR_HIP(hipMemsetAsync(a->dL_dcampos, 0, sizeof(float) * 3, stream));
    return GSR_OK;
}

// The background's gradients (gsr_composite_ext), written with the composite: one pass over final_T (null: no Gaussian,
// T = 1) and dL_dpix on the caller's stream, its per-workgroup partials in the caller's GSR_BUF_BACKGROUND_PARTIALS
static int background_grads(const gsr_backward_args *a, const CompositeExt &e, const float *final_T, gsr_alloc_fn alloc,
                            void *alloc_ctx, hipStream_t stream) {
    if (!e.dL_dbackground && !e.dL_dbackground_image) return GSR_OK;
    const size_t HW = (size_t)a->W * a->H;
    float *partials = nullptr;
    if (e.dL_dbackground) {
        partials = reinterpret_cast<float *>(alloc(alloc_ctx, GSR_BUF_BACKGROUND_PARTIALS, background_partials_bytes(HW)));
        if (!partials) return fail(GSR_ERR_ALLOC, "background partials allocation failed");
    }
    GSR_STAGE(ST_BACKGROUND_GRAD, a->debug != 0,
              launch_background_grad(stream, HW, final_T, a->dL_dpix, e.dL_dbackground_image, e.dL_dbackground, partials));
    return GSR_OK;
}

// One backward call's state: what the argument checks read and derived, the forward's state recovered from its buffers,
// and what one stage leaves for the next.  Each stage below takes it whole.
struct BwdCall : RasterState {
    const gsr_backward_args *a;
    gsr_alloc_fn alloc;
    void *alloc_ctx;
    hipStream_t stream;
    bool dbg;
    CompositeExt e;
    AbsgradExt ab;
    FeaturesExt fx;
    bool feat_bwd;   // the feature work of this call: only with an upstream gradient of the feature image
    DistortionExt dx;
    bool dist_bwd;   // the distortion work of this call: only with an upstream gradient of the map
    MedianExt mx;
    bool med_bwd;    // the median work of this call: only with an upstream gradient of the median depth
    int64_t g0, g1;  // the Gaussians of the per-Gaussian stage
    BwdScratch sc;
    GatherSrc src;   // what every gather of this call tests (live: null with "bwd_live" 0, decided once)
    bool prezeroed;  // the composite zero-filled the per-Gaussian outputs (zero_fill_plan), and did launch
};

// The side structs and every argument check, in the order callers see their errors.  With P == 0 it ends after the
// checks an empty scene needs (as check_common does).
static int bwd_check_args(BwdCall &c, const gsr_composite_ext *ext, const gsr_absgrad_ext *absgrad,
                          const gsr_features_ext *feat, const gsr_distortion_ext *dist, const gsr_median_ext *median) {
    const gsr_backward_args *a = c.a;
    int rc = read_composite_ext(ext, a->background, c.e);
    if (rc) return rc;
    read_absgrad_ext(absgrad, c.ab);
    rc = read_features_ext(feat, a->P, c.fx);
    if (rc) return rc;
    if (c.fx.given && c.ab.dL_dmeans2D_abs)
        return fail(GSR_ERR_UNSUPPORTED, "features with gsr_absgrad_ext.dL_dmeans2D_abs are not built yet");
    if (c.fx.given && a->stages != GSR_BWD_ALL)
        return fail(GSR_ERR_UNSUPPORTED, "features with a split backward (stages != GSR_BWD_ALL) are not built yet");
    c.feat_bwd = c.fx.given && c.fx.dL_dout_features != nullptr;
    rc = read_distortion_ext(dist, c.dx);
    if (rc) return rc;
    if (c.dx.given && c.ab.dL_dmeans2D_abs)
        return fail(GSR_ERR_UNSUPPORTED, "distortion with gsr_absgrad_ext.dL_dmeans2D_abs is not built");
    if (c.dx.given && a->stages != GSR_BWD_ALL)
        return fail(GSR_ERR_UNSUPPORTED, "distortion with a split backward (stages != GSR_BWD_ALL) is not built");
    c.dist_bwd = c.dx.given && c.dx.dL_dD != nullptr;
    rc = read_median_ext(median, c.mx);
    if (rc) return rc;
    if (c.mx.given && c.ab.dL_dmeans2D_abs)
        return fail(GSR_ERR_UNSUPPORTED, "median depth with gsr_absgrad_ext.dL_dmeans2D_abs is not built");
    if (c.mx.given && a->stages != GSR_BWD_ALL)
        return fail(GSR_ERR_UNSUPPORTED, "median depth with a split backward (stages != GSR_BWD_ALL) is not built");
    c.med_bwd = c.mx.given && c.mx.dL_dmedian != nullptr;
    if (c.ab.densify_abs && !a->densify_stats)
        return fail(GSR_ERR_ARG, "gsr_absgrad_ext.densify_abs needs densify_stats");
    if (c.ab.densify_abs && !c.ab.dL_dmeans2D_abs)
        return fail(GSR_ERR_ARG, "gsr_absgrad_ext.densify_abs needs dL_dmeans2D_abs");
    if (a->stages == GSR_BWD_GAUSSIANS)  // the per-Gaussian stage reads no background: only its presence counts
        c.e.out_alpha = nullptr, c.e.dL_dalpha = nullptr, c.e.dL_dbackground = c.e.dL_dbackground_image = nullptr;
    rc = check_common(a->P, a->D, a->M, a->W, a->H, a->means3D, a->opacities, a->colors_precomp, a->shs,
                      a->scales, a->rotations, a->cov3D_precomp, a->viewmatrix, a->projmatrix, a->campos,
                      c.e.background_image ? c.e.background_image : a->background);
    if (rc) return rc;
    if ((c.e.dL_dbackground || c.e.dL_dbackground_image) && !a->dL_dpix)
        return fail(GSR_ERR_ARG, "dL_dpix is required for the background gradients");
    if (a->P == 0) return GSR_OK;
    if (!a->dL_dpix || !a->radii) return fail(GSR_ERR_ARG, "dL_dpix and radii are required");
    if (!a->geom_buffer || !a->image_buffer || (a->R > 0 && !a->binning_buffer))
        return fail(GSR_ERR_ARG, "forward buffers are required");
    if (a->stages != GSR_BWD_COMPOSITE && a->shs && a->M > 0 && !a->dL_dsh && !a->dL_dcolors_sh)
        return fail(GSR_ERR_ARG, "dL_dsh (or dL_dcolors_sh) is required when shs are given");
    if (a->R < 0 || a->R > 0xffffffffLL) return fail(GSR_ERR_ARG, "bad num_rendered");
    if (a->stages < GSR_BWD_ALL || a->stages > GSR_BWD_GAUSSIANS) return fail(GSR_ERR_ARG, "bad backward stages");
    if (a->campos_rows && (!a->campos || a->campos_nrows < 1 || a->campos_rank < 0 || a->campos_rank >= a->campos_nrows))
        return fail(GSR_ERR_ARG, "campos_rows needs campos and 0 <= campos_rank < campos_nrows");
    c.g0 = a->g_begin, c.g1 = a->g_end;
    if (c.g0 == 0 && c.g1 == 0) c.g1 = a->P;
    if (c.g0 < 0 || c.g1 < c.g0 || c.g1 > a->P) return fail(GSR_ERR_ARG, "bad Gaussian range [g_begin, g_end)");
    if (a->stages == GSR_BWD_GAUSSIANS && a->R > 0 && !a->bwd_scratch)
        return fail(GSR_ERR_ARG, "GSR_BWD_GAUSSIANS needs the bwd_scratch of the GSR_BWD_COMPOSITE call");
    if (a->num_big > a->P) return fail(GSR_ERR_ARG, "bad num_big");
    return GSR_OK;
}

// The forward's buffers and this call's scratch (allocated here, or the composite call's for GSR_BWD_GAUSSIANS), carved
static int bwd_carve(BwdCall &c) {
    const gsr_backward_args *a = c.a;
    recover_state(c, a->P, a->W, a->H, a->R, a->num_big, a->geom_buffer, a->binning_buffer, a->image_buffer);
    const bool abs = c.ab.dL_dmeans2D_abs != nullptr;
    const int fb = c.feat_bwd ? feat_block(c.fx.C) : 0;
    char *scratch = a->bwd_scratch;
    if (a->stages != GSR_BWD_GAUSSIANS) {
        scratch = c.alloc(c.alloc_ctx, GSR_BUF_BWD_SCRATCH, bwd_scratch_size(c.R, c.nbig, abs, fb));
        if (!scratch) return fail(GSR_ERR_ALLOC, "backward scratch allocation failed");
    }
    carve_bwd_scratch(scratch, c.R, c.nbig, abs, fb, c.sc);
    c.src = gather_src(a->radii, c, true, tuning(K_bwd_live) != 0);
    return GSR_OK;
}

// Compositing backward: the instance gradient rows (and abs rows), the live flags, the zero fill of the outputs
static int bwd_composite(BwdCall &c) {
    const gsr_backward_args *a = c.a;
    hipStream_t stream = c.stream;
    RenderBwdParams rp;
    rp.W = a->W; rp.H = a->H; rp.gx = c.gx; rp.gy = c.gy; rp.num_tiles = (int)c.T; rp.num_rendered = c.R;
    rp.ranges = c.im.ranges; rp.point_list = c.b.point_list; rp.n_contrib = c.im.n_contrib;
    const int lpt = tuning(K_lpt);
    // the backward's own order (by tile_last; reusing the forward's range-length order measured slower)
    const bool own_order = lpt != 0;
    // in lpt_append_range the forward's whole-tile waves filled the bucket lists (render_bwd falls back to the
    // identity order if that forward did not, *lpt_valid = 0: the order never changes a result)
    const bool lists = own_order && lpt_append_range(c.T);
    if (own_order && !lists)
        launch_tile_order(stream, c.im.ranges, c.im.tile_last, 1, (int)c.T, c.im.order_bwd, c.im.lpt_hist);
    rp.tile_order = lpt ? (own_order ? (lists ? nullptr : c.im.order_bwd) : c.im.order_fwd) : nullptr;
    if (lists) {
        rp.lpt_bcnt = c.im.lpt_bcnt; rp.lpt_blist = c.im.lpt_blist; rp.lpt_valid = c.im.lpt_valid;
    }
    rp.tile_last = c.im.tile_last; rp.tile_loaded = c.im.tile_loaded;
    rp.rec = c.g.rec;
    rp.bg = a->background ? a->background : c.e.background_image; rp.bg_image = c.e.background_image;
    rp.dL_dalpha = c.e.dL_dalpha;
    rp.final_T = c.im.final_T; rp.dL_dpix = a->dL_dpix; rp.dL_dinvdepth = a->dL_dinvdepth;
    rp.rows = c.sc.rows;
    rp.abs_rows = c.sc.abs_rows;
    rp.live = c.src.live ? c.g.live : nullptr;
    rp.live_valid = c.g.counters + CNT_LIVE_VALID;
    rp.sorted_u = c.b.sorted_u;
    rp.strip_mask = c.b.strip_mask; rp.smask_valid = c.im.smask_valid;
    if (c.T <= SEG_MAX_TILES && tuning(K_bwd_seg)) {  // segmented walk (from the forward's checkpoints, if any)
        rp.ckpt = c.b.ckpt; rp.ctot = c.im.ctot; rp.ck_flag = c.im.ck_flag;
        rp.seg_list = c.b.seg_list; rp.seg_count = c.im.seg_count;
    }
    const bool planned = a->stages == GSR_BWD_ALL && tuning(K_bwd_prezero) &&
                         zero_fill_plan(a, c.ab.dL_dmeans2D_abs, c.g0, c.g1, rp);
    bool launched = false;
    GSR_STAGE(ST_RENDER_BWD, c.dbg, launched = launch_render_bwd(stream, rp));
    c.prezeroed = planned && launched;  // (the fill is the composite's: no launch, no zeros)
    return GSR_OK;
}

// Channel block after channel block: the walk adds the block's geometry terms into the rows render_bwd just wrote (and
// marks the live flags), then the block's feature rows are gathered into dL_dfeatures, so one block's rows are all the
// scratch there is.  big_reduce then sums rows that hold every term.
static int bwd_features(BwdCall &c) {
    const gsr_backward_args *a = c.a;
    hipStream_t stream = c.stream;
    FeatBwdParams fp;
    fp.src = replay_src(c);
    fp.C = c.fx.C;
    fp.final_T = c.im.final_T; fp.features = c.fx.features; fp.dL_dF = c.fx.dL_dout_features;
    fp.rows = c.sc.rows; fp.frows = c.sc.feat_rows;
    fp.live = c.src.live ? c.g.live : nullptr;
    FeatGatherParams gp;
    gp.P = a->P; gp.C = c.fx.C;
    gp.src = c.src;
    gp.frows = c.sc.feat_rows; gp.bigsum = c.sc.feat_bigsum;
    gp.nbig = c.nbig; gp.nbig_dev = c.nbig_dev;
    gp.out = c.fx.dL_dfeatures;
    const int fb = feat_block(c.fx.C);
    for (int c0 = 0; c0 < c.fx.C; c0 += fb) {
        fp.c0 = gp.c0 = c0;
        GSR_STAGE(ST_FEAT_BWD, c.dbg, launch_feat_bwd(stream, fp));
        if (gp.out) GSR_STAGE(ST_FEAT_GATHER, c.dbg, launch_feat_gather(stream, gp));
    }
    return GSR_OK;
}

// The distortion walk adds its geometry terms and, as inverse-depth weight, its depth term into the rows (and marks
// the live flags): big_reduce and the per-Gaussian stage then see rows that hold every term
static int bwd_distortion(BwdCall &c) {
    hipStream_t stream = c.stream;
    DistBwdParams dp;
    dp.src = replay_src(c);
    dp.depth_key = c.g.depth_key;
    dp.map = c.dx.map; dp.k0 = dist_k0(c.dx); dp.nearp = c.dx.nearp; dp.dscale = dist_dscale(c.dx);
    dp.final_T = c.im.final_T; dp.tot_w = c.dx.tot_w; dp.tot_m = c.dx.tot_m; dp.dL_dD = c.dx.dL_dD;
    dp.rows = c.sc.rows;
    dp.live = c.src.live ? c.g.live : nullptr;
    GSR_STAGE(ST_DIST_BWD, c.dbg, launch_dist_bwd(stream, dp));
    return GSR_OK;
}

// The median walk adds, as inverse-depth weight, each selected instance's summed upstream gradient into the rows (and
// marks the live flags)
static int bwd_median(BwdCall &c) {
    hipStream_t stream = c.stream;
    MedianBwdParams mp;
    mp.src = replay_src(c);
    mp.depth_key = c.g.depth_key;
    mp.pos = c.mx.pos; mp.dL_dmedian = c.mx.dL_dmedian;
    mp.rows = c.sc.rows;
    mp.live = c.src.live ? c.g.live : nullptr;
    GSR_STAGE(ST_MEDIAN_BWD, c.dbg, launch_median_bwd(stream, mp));
    return GSR_OK;
}

// The big Gaussians' rows (and abs rows), summed by a workgroup each
static int bwd_big_reduce(BwdCall &c) {
    hipStream_t stream = c.stream;
    BigReduceParams bp;
    bp.src = c.src;
    bp.rows = c.sc.rows; bp.bigsum = c.sc.bigsum;
    bp.abs_rows = c.sc.abs_rows; bp.bigsum_abs = c.sc.bigsum_abs;
    bp.nbig_dev = c.nbig_dev;
    GSR_STAGE(ST_BIG_REDUCE, c.dbg, launch_big_reduce(stream, bp, c.nbig));
    return GSR_OK;
}

// Per-Gaussian stage over [g0, g1): the rows gathered, the preprocess backward, the camera sums, the abs gather
static int bwd_gaussians(BwdCall &c) {
    const gsr_backward_args *a = c.a;
    hipStream_t stream = c.stream;
    const int64_t g0 = c.g0, g1 = c.g1;
    // Chunk-relative outputs (a split backward) address Gaussian g0's row: shift them so the kernel indexes every
    // output by the absolute Gaussian index (integer arithmetic: the shifted address is never dereferenced)
    auto rel = [g0](auto *ptr, int64_t width) -> decltype(ptr) {
        if (!ptr || g0 == 0) return ptr;
        return reinterpret_cast<decltype(ptr)>(reinterpret_cast<uintptr_t>(ptr) - (uintptr_t)(g0 * width) * sizeof(*ptr));
    };
    PreprocessBwdParams pp;
    pp.P = a->P; pp.D = a->D; pp.M = a->M; pp.W = a->W; pp.H = a->H;
    pp.g0 = (int)g0; pp.g1 = (int)g1;
    pp.tan_fovx = a->tan_fovx; pp.tan_fovy = a->tan_fovy;
    pp.focal_x = a->W / (2.0f * a->tan_fovx);
    pp.focal_y = a->H / (2.0f * a->tan_fovy);
    pp.scale_modifier = a->scale_modifier;
    pp.antialiasing = a->antialiasing;
    pp.has_invdepth = a->dL_dinvdepth != nullptr || ((c.dist_bwd || c.med_bwd) && c.R > 0);  // (the distortion's depth term, the median's: rows[..][9])
    pp.means3D = a->means3D; pp.opacities = a->opacities; pp.scales = a->scales; pp.rotations = a->rotations;
    pp.cov3D_precomp = a->cov3D_precomp; pp.shs = (a->colors_precomp ? nullptr : a->shs);
    pp.view = a->viewmatrix; pp.proj = a->projmatrix; pp.campos = a->campos;
    pp.src = c.src;
    pp.clamped = c.g.clamped;
    pp.sh_jac = c.g.sh_jac;  // the forward's d rgb / d dir: the SH term of dL/dmeans3D reads no coefficient
    pp.bigsum = c.sc.bigsum;
    pp.rows = c.sc.rows;
    pp.sh_vec16 = pp.shs && a->M == 16 && (((uintptr_t)pp.shs | (uintptr_t)a->dL_dsh) & 15) == 0;
    pp.dL_dmeans2D = rel(a->dL_dmeans2D, 3); pp.dL_dcolors = rel(a->dL_dcolors, 3);
    pp.dL_dopacity = rel(a->dL_dopacity, 1); pp.dL_dmeans3D = rel(a->dL_dmeans3D, 3);
    pp.dL_dcov3D = rel(a->dL_dcov3D, 6); pp.dL_dsh = rel(a->dL_dsh, (int64_t)a->M * 3);
    pp.dL_dcolors_sh = rel(a->dL_dcolors_sh, 3);
    pp.densify_stats = c.ab.densify_abs ? nullptr : rel(a->densify_stats, 2);  // (densify_abs: written by the abs gather)
    pp.densify_accumulate = a->densify_accumulate;
    pp.max_radii2D = rel(a->max_radii2D, 1);
    pp.dL_dscales = rel(a->dL_dscales, 3); pp.dL_drot = rel(a->dL_drotations, 4);
    pp.campos_rows = a->campos_rows; pp.campos_rank = a->campos_rank; pp.campos_nrows = a->campos_nrows;
    pp.prezeroed = c.prezeroed ? 1 : 0;
    const size_t ng = (size_t)(g1 - g0);
    if (pp.shs == nullptr && a->dL_dsh && a->M > 0)
        GSR_HIP(hipMemsetAsync(a->dL_dsh, 0, sizeof(float) * ng * a->M * 3, stream));
    if (pp.shs == nullptr && a->dL_dcolors_sh)
        GSR_HIP(hipMemsetAsync(a->dL_dcolors_sh, 0, sizeof(float) * ng * 3, stream));
    if (camera_grads(a)) {
        if (ng == 0) return zero_camera_grads(a, stream);
        pp.cam_partials = reinterpret_cast<float *>(c.alloc(c.alloc_ctx, GSR_BUF_CAMERA_PARTIALS, camera_partials_bytes((int64_t)ng)));
        if (!pp.cam_partials) return fail(GSR_ERR_ALLOC, "camera partials allocation failed");
    }
    AbsGatherParams gp{};
    if (c.ab.dL_dmeans2D_abs) {
        gp.g0 = (int)g0; gp.g1 = (int)g1;
        gp.src = c.src;
        gp.abs_rows = c.sc.abs_rows; gp.bigsum_abs = c.sc.bigsum_abs;
        gp.out = rel(c.ab.dL_dmeans2D_abs, 2);
        gp.densify_stats = c.ab.densify_abs ? rel(a->densify_stats, 2) : nullptr;
        gp.densify_accumulate = a->densify_accumulate;
        gp.prezeroed = pp.prezeroed;
    }
    GSR_STAGE(ST_PREPROCESS_BWD, c.dbg, {
        launch_preprocess_bwd(stream, pp);
        if (pp.cam_partials) launch_camera_reduce(stream, pp, a->dL_dviewmatrix, a->dL_dprojmatrix, a->dL_dcampos);
        if (c.ab.dL_dmeans2D_abs) launch_abs_gather(stream, gp);
    });
    return GSR_OK;
}

int gsr_backward(const gsr_backward_args *a, gsr_alloc_fn alloc, void *alloc_ctx, void *stream_ptr) {
    return gsr_backward_ext(a, nullptr, alloc, alloc_ctx, stream_ptr);
}

int gsr_backward_ext(const gsr_backward_args *a, const gsr_composite_ext *ext, gsr_alloc_fn alloc, void *alloc_ctx,
                     void *stream_ptr) {
    return gsr_backward_abs(a, ext, nullptr, alloc, alloc_ctx, stream_ptr);
}

int gsr_backward_abs(const gsr_backward_args *a, const gsr_composite_ext *ext, const gsr_absgrad_ext *absgrad,
                     gsr_alloc_fn alloc, void *alloc_ctx, void *stream_ptr) {
    return gsr_backward_features(a, ext, absgrad, nullptr, alloc, alloc_ctx, stream_ptr);
}

int gsr_backward_features(const gsr_backward_args *a, const gsr_composite_ext *ext, const gsr_absgrad_ext *absgrad,
                          const gsr_features_ext *feat, gsr_alloc_fn alloc, void *alloc_ctx, void *stream_ptr) {
    return gsr_backward_distortion(a, ext, absgrad, feat, nullptr, alloc, alloc_ctx, stream_ptr);
}

int gsr_backward_distortion(const gsr_backward_args *a, const gsr_composite_ext *ext, const gsr_absgrad_ext *absgrad,
                            const gsr_features_ext *feat, const gsr_distortion_ext *dist, gsr_alloc_fn alloc,
                            void *alloc_ctx, void *stream_ptr) {
    return gsr_backward_median(a, ext, absgrad, feat, dist, nullptr, alloc, alloc_ctx, stream_ptr);
}

int gsr_backward_median(const gsr_backward_args *a, const gsr_composite_ext *ext, const gsr_absgrad_ext *absgrad,
                        const gsr_features_ext *feat, const gsr_distortion_ext *dist, const gsr_median_ext *median,
                        gsr_alloc_fn alloc, void *alloc_ctx, void *stream_ptr) {
    if (!a || !alloc) return fail(GSR_ERR_ARG, "null argument");
    BwdCall c{};
    c.a = a; c.alloc = alloc; c.alloc_ctx = alloc_ctx;
    c.stream = (hipStream_t)stream_ptr; c.dbg = a->debug != 0;
    hipStream_t stream = c.stream;
    int rc = bwd_check_args(c, ext, absgrad, feat, dist, median);
    if (rc) return rc;
    if (a->P == 0) {  // no Gaussian: the background's gradients with T_final = 1, the camera's empty sums
        if (!camera_grads(a) && !c.e.dL_dbackground && !c.e.dL_dbackground_image) return GSR_OK;
        StreamDeviceGuard device_guard(stream);
        rc = background_grads(a, c.e, nullptr, alloc, alloc_ctx, stream);
        if (rc) return rc;
        return camera_grads(a) ? zero_camera_grads(a, stream) : GSR_OK;
    }
    StreamDeviceGuard device_guard(stream);
    rc = bwd_carve(c);
    if (rc) return rc;
    if (a->stages != GSR_BWD_GAUSSIANS) {
        if (c.R > 0) {
            rc = bwd_composite(c);
            if (!rc && c.feat_bwd) rc = bwd_features(c);
            if (!rc && c.dist_bwd) rc = bwd_distortion(c);
            if (!rc && c.med_bwd) rc = bwd_median(c);
            if (!rc) rc = bwd_big_reduce(c);
            if (rc) return rc;
        }
        // (with nothing rendered the forward left final_T = 1 everywhere)
        rc = background_grads(a, c.e, c.im.final_T, alloc, alloc_ctx, stream);
        if (rc) return rc;
    }
    if (c.fx.dL_dfeatures && !(c.feat_bwd && c.R > 0))  // no upstream gradient, or nothing rendered: the empty sums
        GSR_HIP(hipMemsetAsync(c.fx.dL_dfeatures, 0, sizeof(float) * (size_t)a->P * c.fx.C, stream));
    if (a->stages == GSR_BWD_COMPOSITE) return GSR_OK;
    return bwd_gaussians(c);
}

int gsr_contributions(const gsr_contrib_args *x, gsr_alloc_fn alloc, void *alloc_ctx, void *stream_ptr) {
    if (!x || !alloc) return fail(GSR_ERR_ARG, "null argument");
    const VersionedIn<gsr_contrib_args> in(x);
    if (!in.covers(&gsr_contrib_args::radii))
        return fail(GSR_ERR_ARG, "gsr_contrib_args: struct_size ends before the first pointer field");
    const int P = in.get(&gsr_contrib_args::P), W = in.get(&gsr_contrib_args::W), H = in.get(&gsr_contrib_args::H);
    const int64_t R = in.get(&gsr_contrib_args::R), num_big = in.get(&gsr_contrib_args::num_big);
    const int32_t *radii = in.get(&gsr_contrib_args::radii);
    const void *geom = in.get(&gsr_contrib_args::geom_buffer), *binning = in.get(&gsr_contrib_args::binning_buffer);
    const void *image = in.get(&gsr_contrib_args::image_buffer);
    int64_t *count = in.get(&gsr_contrib_args::count);
    float *wsum = in.get(&gsr_contrib_args::wsum), *wmax = in.get(&gsr_contrib_args::wmax);
    const int accumulate = in.get(&gsr_contrib_args::accumulate);
    if (!count && !wsum && !wmax) return fail(GSR_ERR_ARG, "gsr_contributions: no output asked for");
    if (P < 0) return fail(GSR_ERR_ARG, "P must be >= 0");
    if (W <= 0 || H <= 0) return fail(GSR_ERR_ARG, "image_width and image_height must be positive");
    if ((int64_t)W * H > 0x7fffffffLL) return fail(GSR_ERR_ARG, "image too large");
    if (R < 0 || R > 0xffffffffLL) return fail(GSR_ERR_ARG, "bad num_rendered");
    if (num_big > P) return fail(GSR_ERR_ARG, "bad num_big");
    if (R > 0 && (!radii || !geom || !binning || !image)) return fail(GSR_ERR_ARG, "forward buffers are required");
    if (P == 0) return GSR_OK;
    hipStream_t stream = (hipStream_t)stream_ptr;
    StreamDeviceGuard device_guard(stream);
    if (R == 0) {  // everything culled: the empty reductions (nothing to add under accumulate)
        if (accumulate) return GSR_OK;
        if (count) GSR_HIP(hipMemsetAsync(count, 0, sizeof(int64_t) * (size_t)P, stream));
        if (wsum) GSR_HIP(hipMemsetAsync(wsum, 0, sizeof(float) * (size_t)P, stream));
        if (wmax) GSR_HIP(hipMemsetAsync(wmax, 0, sizeof(float) * (size_t)P, stream));
        return GSR_OK;
    }
    RasterState st;
    recover_state(st, P, W, H, R, num_big, geom, binning, image);
    char *scratch = alloc(alloc_ctx, GSR_BUF_CONTRIB_SCRATCH, gsr_contrib_scratch_bytes(R, num_big));
    if (!scratch) return fail(GSR_ERR_ALLOC, "contribution scratch allocation failed");
    uint4 *rows, *bigsum;
    carve_contrib_scratch(scratch, R, num_big, &rows, &bigsum);
    ContribWalkParams wp;
    wp.src = replay_src(st);
    wp.pixel_weights = in.get(&gsr_contrib_args::pixel_weights); wp.rows = rows;
    ContribGatherParams gp;
    gp.P = P;
    gp.src = gather_src(radii, st, false, false);  // the live flags are the backward composite's: not valid here
    gp.rows = rows; gp.bigsum = bigsum;
    gp.nbig = st.nbig; gp.nbig_dev = st.nbig_dev;
    gp.count = count; gp.wsum = wsum; gp.wmax = wmax; gp.accumulate = accumulate;
    GSR_STAGE(ST_CONTRIB_WALK, false, launch_contrib_walk(stream, wp));
    GSR_STAGE(ST_CONTRIB_GATHER, false, {
        launch_contrib_big_reduce(stream, gp);
        launch_contrib_gather(stream, gp);
    });
    return GSR_OK;
}

int gsr_sh_backward_views_chunked(int P, int D, int M, int V, int64_t chunk_len, const float *means3D,
                                  const float *campos, const float *dL_dcolors_sh, float *dL_dsh, void *stream_ptr) {
    if (P < 0 || V < 0) return fail(GSR_ERR_ARG, "P and V must be >= 0");
    if (D < 0 || D > 3) return fail(GSR_ERR_ARG, "sh_degree must be in [0, 3]");
    if (M <= 0 || M > 16 || (D + 1) * (D + 1) > M)
        return fail(GSR_ERR_ARG, "M must hold (deg+1)^2 <= M <= 16 coefficients");
    if (chunk_len < 0) return fail(GSR_ERR_ARG, "chunk_len must be >= 0");
    if (P == 0) return GSR_OK;
    if (!means3D || !dL_dsh || (V > 0 && (!campos || !dL_dcolors_sh))) return fail(GSR_ERR_ARG, "null argument");
    hipStream_t stream = (hipStream_t)stream_ptr;
    StreamDeviceGuard device_guard(stream);
    const int L = (chunk_len == 0 || chunk_len >= P) ? P : (int)chunk_len;
    GSR_STAGE(ST_SH_VIEWS, 0, launch_sh_backward_views(stream, P, D, M, V, L, means3D, campos, dL_dcolors_sh, dL_dsh));
    return GSR_OK;
}

int gsr_sh_backward_views(int P, int D, int M, int V, const float *means3D, const float *campos,
                          const float *dL_dcolors_sh, float *dL_dsh, void *stream_ptr) {
    return gsr_sh_backward_views_chunked(P, D, M, V, 0, means3D, campos, dL_dcolors_sh, dL_dsh, stream_ptr);
}

int gsr_adam_sh_views_step(const gsr_adam_sh_views_args *a, double beta1, double beta2, double eps, void *stream_ptr) {
    if (!a) return fail(GSR_ERR_ARG, "adam sh views: null arguments");
    if (a->P < 0 || a->V < 0) return fail(GSR_ERR_ARG, "P and V must be >= 0");
    if (a->D < 0 || a->D > 3) return fail(GSR_ERR_ARG, "sh_degree must be in [0, 3]");
    if (a->M != 16) return fail(GSR_ERR_ARG, "adam sh views: M must be 16");
    if (a->chunk_len < 0) return fail(GSR_ERR_ARG, "chunk_len must be >= 0");
    if (a->dc_step < 1 || a->rest_step < 1) return fail(GSR_ERR_ARG, "adam: step must be >= 1");
    if (a->P == 0) return GSR_OK;
    if (!a->means3D || (a->V > 0 && (!a->campos || !a->dL_dcolors_sh)) || !a->dc_param || !a->dc_exp_avg ||
        !a->dc_exp_avg_sq || !a->rest_param || !a->rest_exp_avg || !a->rest_exp_avg_sq)
        return fail(GSR_ERR_ARG, "null argument");
    AdamShLaunch L{};
    L.P = a->P; L.V = a->V;
    L.L = (a->chunk_len == 0 || a->chunk_len >= a->P) ? a->P : (int)a->chunk_len;
    L.means3D = a->means3D; L.campos = a->campos; L.dc = a->dL_dcolors_sh;
    if ((a->param_row_stride != 0 && a->param_row_stride != 48) || (a->moment_row_stride != 0 && a->moment_row_stride != 48))
        return fail(GSR_ERR_ARG, "adam sh views: row strides must be 0 (packed) or 48 (one (P, 16, 3) tensor)");
    if (a->moment_row_stride == 48 && a->param_row_stride != 48)
        return fail(GSR_ERR_ARG, "adam sh views: joint moments need the joint parameter");
    if (a->param_row_stride == 48 && (a->rest_param != a->dc_param + 3 ||
                                      (a->moment_row_stride == 48 && (a->rest_exp_avg != a->dc_exp_avg + 3 ||
                                                                      a->rest_exp_avg_sq != a->dc_exp_avg_sq + 3))))
        return fail(GSR_ERR_ARG, "adam sh views: a joint tensor's rest block must start 3 floats after its dc block");
    auto group = [&](AdamShGroup &g, float *p, float *m, float *v, double lr, int64_t step, int64_t width) {
        const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
        g.param = p; g.exp_avg = m; g.exp_avg_sq = v;
        g.param_stride = a->param_row_stride ? a->param_row_stride : width;
        g.step_size = (float)(lr / bc1);  // as gsr_adam_step
        g.bc2_sqrt = (float)std::sqrt(bc2);
    };
    group(L.dc_group, a->dc_param, a->dc_exp_avg, a->dc_exp_avg_sq, a->dc_lr, a->dc_step, 3);
    group(L.rest_group, a->rest_param, a->rest_exp_avg, a->rest_exp_avg_sq, a->rest_lr, a->rest_step, 45);
    // float4 moments (and parameters when packed) need 16-B aligned bases
    const uintptr_t params = a->param_row_stride ? 0 : (((uintptr_t)a->dc_param) | ((uintptr_t)a->rest_param));
    L.vec4 = ((params | ((uintptr_t)a->dc_exp_avg) | ((uintptr_t)a->dc_exp_avg_sq) | ((uintptr_t)a->rest_exp_avg) |
               ((uintptr_t)a->rest_exp_avg_sq)) & 15) == 0;
    L.one_minus_beta1 = (float)(1.0 - beta1);
    L.beta2 = (float)beta2;
    L.one_minus_beta2 = (float)(1.0 - beta2);
    L.eps = (float)eps;
    L.joint = a->moment_row_stride == 48 &&
              ((((uintptr_t)a->dc_param) | ((uintptr_t)a->dc_exp_avg) | ((uintptr_t)a->dc_exp_avg_sq)) & 15) == 0;
    hipStream_t stream = (hipStream_t)stream_ptr;
    StreamDeviceGuard device_guard(stream);
    GSR_STAGE(ST_ADAM_SH, 0, launch_adam_sh_views(stream, L, a->D));
    return GSR_OK;
}

int gsr_adam_step(const gsr_adam_group *groups, int num_groups, double beta1, double beta2, double eps,
                  void *stream_ptr) {
    if (num_groups < 0 || num_groups > ADAM_MAX_GROUPS) return fail(GSR_ERR_ARG, "adam: 0..16 parameter groups");
    if (num_groups && !groups) return fail(GSR_ERR_ARG, "adam: null groups");
    AdamLaunch L{};
    int64_t slices = 0;
    int ng = 0;
    for (int i = 0; i < num_groups; i++) {
        const gsr_adam_group &g = groups[i];
        if (g.n < 0 || g.step < 1) return fail(GSR_ERR_ARG, "adam: n must be >= 0 and step >= 1");
        if (g.n == 0) continue;
        if (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq) return fail(GSR_ERR_ARG, "adam: null array");
        AdamGroupDev &d = L.g[ng];
        d.param = g.param; d.grad = g.grad; d.exp_avg = g.exp_avg; d.exp_avg_sq = g.exp_avg_sq; d.n = g.n;
        const double bc1 = 1.0 - std::pow(beta1, (double)g.step), bc2 = 1.0 - std::pow(beta2, (double)g.step);
        d.step_size = (float)(g.lr / bc1);
        d.bc2_sqrt = (float)std::sqrt(bc2);
        d.vec4 = ((((uintptr_t)g.param) | ((uintptr_t)g.grad) | ((uintptr_t)g.exp_avg) |
                   ((uintptr_t)g.exp_avg_sq)) & 15) == 0;
        L.slice_start[ng] = slices;
        slices += adam_slices(g.n);
        ng++;
    }
    if (slices > 0x7fffffffLL) return fail(GSR_ERR_ARG, "adam: too many elements");
    L.num_groups = ng;
    L.one_minus_beta1 = (float)(1.0 - beta1);
    L.beta2 = (float)beta2;
    L.one_minus_beta2 = (float)(1.0 - beta2);
    L.eps = (float)eps;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_adam((hipStream_t)stream_ptr, L, slices);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

static bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

int gsr_activations_forward(int64_t N, const float *scaling, const float *opacity, const float *rotation,
                            float *scales, float *opacities, float *rotations, void *stream_ptr) {
    if (N < 0 || N > 0x7fffffffLL * 256) return fail(GSR_ERR_ARG, "activations: bad N");
    if (N == 0) return GSR_OK;
    if (!scaling || !opacity || !rotation || !scales || !opacities || !rotations)
        return fail(GSR_ERR_ARG, "activations: null array");
    if (!aligned16(rotation) || !aligned16(rotations)) return fail(GSR_ERR_ARG, "activations: rotation arrays must be 16-B aligned");
    ActivationArgs A{};
    A.N = N;
    A.scaling = scaling; A.opacity = opacity; A.rotation = rotation;
    A.scales = scales; A.opacities = opacities; A.rotations = rotations;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_activations_forward((hipStream_t)stream_ptr, A);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_activations_backward(int64_t N, const float *rotation, const float *scales, const float *opacities,
                             const float *rotations, const float *dL_dscales, const float *dL_dopacities,
                             const float *dL_drotations, float *dL_dscaling, float *dL_dopacity, float *dL_drotation,
                             void *stream_ptr) {
    if (N < 0 || N > 0x7fffffffLL * 256) return fail(GSR_ERR_ARG, "activations: bad N");
    if (N == 0) return GSR_OK;
    if (!rotation || !scales || !opacities || !rotations || !dL_dscales || !dL_dopacities || !dL_drotations ||
        !dL_dscaling || !dL_dopacity || !dL_drotation)
        return fail(GSR_ERR_ARG, "activations: null array");
    if (!aligned16(rotation) || !aligned16(rotations) || !aligned16(dL_drotations) || !aligned16(dL_drotation))
        return fail(GSR_ERR_ARG, "activations: rotation arrays must be 16-B aligned");
    ActivationArgs A{};
    A.N = N;
    A.rotation = rotation;
    A.scales = const_cast<float *>(scales); A.opacities = const_cast<float *>(opacities);
    A.rotations = const_cast<float *>(rotations);
    A.dL_dscales = dL_dscales; A.dL_dopacities = dL_dopacities; A.dL_drotations = dL_drotations;
    A.dL_dscaling = dL_dscaling; A.dL_dopacity = dL_dopacity; A.dL_drotation = dL_drotation;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_activations_backward((hipStream_t)stream_ptr, A);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_sparse_adam_step(const gsr_adam_group *groups, int num_groups, const uint8_t *visible, int64_t N,
                         double beta1, double beta2, double eps, void *stream_ptr) {
    if (num_groups < 0 || num_groups > ADAM_MAX_GROUPS) return fail(GSR_ERR_ARG, "sparse adam: 0..16 parameter groups");
    if (num_groups && !groups) return fail(GSR_ERR_ARG, "sparse adam: null groups");
    if (N <= 0) return fail(GSR_ERR_ARG, "sparse adam: N must be positive");
    if (!visible) return fail(GSR_ERR_ARG, "sparse adam: null visibility");
    AdamLaunch L{};
    int64_t slices = 0;
    int ng = 0;
    for (int i = 0; i < num_groups; i++) {
        const gsr_adam_group &g = groups[i];
        if (g.n < 0) return fail(GSR_ERR_ARG, "sparse adam: n must be >= 0");
        if (g.n == 0) continue;
        if (g.n % N != 0) return fail(GSR_ERR_ARG, "sparse adam: a group's element count is not a multiple of N");
        if (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq) return fail(GSR_ERR_ARG, "sparse adam: null array");
        AdamGroupDev &d = L.g[ng];
        d.param = g.param; d.grad = g.grad; d.exp_avg = g.exp_avg; d.exp_avg_sq = g.exp_avg_sq; d.n = g.n;
        d.M = g.n / N;
        d.lr = (float)g.lr;
        d.vec4 = ((((uintptr_t)g.param) | ((uintptr_t)g.grad) | ((uintptr_t)g.exp_avg) |
                   ((uintptr_t)g.exp_avg_sq)) & 15) == 0;
        L.slice_start[ng] = slices;
        slices += adam_slices(g.n);
        ng++;
    }
    if (slices > 0x7fffffffLL) return fail(GSR_ERR_ARG, "sparse adam: too many elements");
    L.num_groups = ng;
    L.beta1 = (float)beta1;
    L.one_minus_beta1 = 1.0f - (float)beta1;  // the upstream kernel forms 1 - b1 in float
    L.beta2 = (float)beta2;
    L.one_minus_beta2 = 1.0f - (float)beta2;
    L.eps = (float)eps;
    L.visible = visible;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_sparse_adam((hipStream_t)stream_ptr, L, slices);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

// densify workspace: [dst_map 2N i32 | split_rank N i32 | block_counts 3*blocks i32 | row_class N u8]
static size_t densify_ws(int64_t N, size_t *o_rank, size_t *o_blk, size_t *o_cls) {
    const size_t nb = (size_t)densify_blocks(N);
    *o_rank = align_up((size_t)N * 8, 256);
    *o_blk = *o_rank + align_up((size_t)N * 4, 256);
    *o_cls = *o_blk + align_up(nb * 12, 256);
    return *o_cls + align_up((size_t)N, 256);
}

size_t gsr_densify_workspace_bytes(int64_t N) {
    size_t a, b, c;
    return N < 0 ? 0 : densify_ws(N, &a, &b, &c);
}

int gsr_densify_classify(const gsr_densify_args *args, void *workspace, int32_t *counts, int64_t *preserve_idx,
                         void *stream_ptr) {
    if (!args || args->N < 0 || args->N > 0x7fffffffLL) return fail(GSR_ERR_ARG, "densify: 0 <= N < 2^31");
    if (!counts) return fail(GSR_ERR_ARG, "densify: null counts");
    DensifyParams p{};
    p.N = args->N;
    if (p.N > 0 && (!args->opacity || !args->scaling || !args->xyz_grad_accum || !args->xyz_grad_count ||
                    !workspace || !preserve_idx || (args->apply_screensize && !args->max_radii2D)))
        return fail(GSR_ERR_ARG, "densify: null input");
    size_t o_rank, o_blk, o_cls;
    densify_ws(p.N, &o_rank, &o_blk, &o_cls);
    char *ws = (char *)workspace;
    p.opacity = args->opacity; p.scaling = args->scaling; p.max_radii2D = args->max_radii2D;
    p.grad_accum = args->xyz_grad_accum; p.grad_count = args->xyz_grad_count;
    p.opacity_threshold = args->opacity_threshold; p.screensize_threshold = args->screensize_threshold;
    p.size_threshold = args->size_threshold; p.grad_threshold = args->grad_threshold;
    p.clone_size_threshold = args->clone_size_threshold;
    p.apply_screensize = args->apply_screensize; p.apply_size = args->apply_size;
    p.dst_map = (int32_t *)ws;
    p.split_rank = (int32_t *)(ws + o_rank);
    p.block_counts = (int32_t *)(ws + o_blk);
    p.row_class = (uint8_t *)(ws + o_cls);
    p.counts = counts;
    p.preserve_idx = preserve_idx;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_densify_classify((hipStream_t)stream_ptr, p);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_densify_classify_keep(int64_t N, const uint8_t *keep_mask, void *workspace, int32_t *counts,
                              int64_t *preserve_idx, void *stream_ptr) {
    if (N < 0 || N > 0x7fffffffLL) return fail(GSR_ERR_ARG, "densify: 0 <= N < 2^31");
    if (!counts) return fail(GSR_ERR_ARG, "densify: null counts");
    if (N > 0 && (!keep_mask || !workspace || !preserve_idx)) return fail(GSR_ERR_ARG, "densify: null input");
    size_t o_rank, o_blk, o_cls;
    densify_ws(N, &o_rank, &o_blk, &o_cls);
    char *ws = (char *)workspace;
    DensifyParams p{};
    p.N = N;
    p.dst_map = (int32_t *)ws;
    p.split_rank = (int32_t *)(ws + o_rank);
    p.block_counts = (int32_t *)(ws + o_blk);
    p.row_class = (uint8_t *)(ws + o_cls);
    p.counts = counts;
    p.preserve_idx = preserve_idx;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_densify_classify_keep((hipStream_t)stream_ptr, p, keep_mask);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_densify_apply(int64_t N, const void *workspace, const float *rotation, const float *scaling, const float *z,
                      const gsr_densify_field *fields, int num_fields, void *stream_ptr) {
    if (N < 0 || N > 0x7fffffffLL) return fail(GSR_ERR_ARG, "densify: 0 <= N < 2^31");
    if (num_fields < 0 || num_fields > DENSIFY_MAX_FIELDS) return fail(GSR_ERR_ARG, "densify: 0..16 fields");
    if (N == 0 || num_fields == 0) return GSR_OK;
    if (!workspace || !fields || !rotation || !scaling) return fail(GSR_ERR_ARG, "densify: null input");
    size_t o_rank, o_blk, o_cls;
    densify_ws(N, &o_rank, &o_blk, &o_cls);
    DensifyApply A{};
    A.N = N;
    A.dst_map = (const int32_t *)workspace;
    A.split_rank = (const int32_t *)((const char *)workspace + o_rank);
    A.z = z; A.rotation = rotation; A.scaling = scaling;
    int64_t blocks = 0;
    for (int i = 0; i < num_fields; i++) {
        const gsr_densify_field &f = fields[i];
        if (f.width <= 0 || !f.src || !f.dst) return fail(GSR_ERR_ARG, "densify: field needs src, dst, width > 0");
        if (f.kind < GSR_FIELD_PLAIN || f.kind > GSR_FIELD_STAT) return fail(GSR_ERR_ARG, "densify: bad kind");
        if (f.kind == GSR_FIELD_XYZ && f.width != 3) return fail(GSR_ERR_ARG, "densify: xyz field width must be 3");
        if ((f.dst_exp_avg && !f.src_exp_avg) || (f.dst_exp_avg_sq && !f.src_exp_avg_sq))
            return fail(GSR_ERR_ARG, "densify: moment destination without source");
        DensifyFieldDev &d = A.f[i];
        d.src = f.src; d.dst = f.dst; d.src_exp_avg = f.src_exp_avg; d.src_exp_avg_sq = f.src_exp_avg_sq;
        d.dst_exp_avg = f.dst_exp_avg; d.dst_exp_avg_sq = f.dst_exp_avg_sq; d.width = f.width; d.kind = f.kind;
        A.block_start[i] = blocks;
        blocks += (N * f.width + 255) / 256;
    }
    if (blocks > 0x7fffffffLL) return fail(GSR_ERR_ARG, "densify: too many elements");
    A.num_fields = num_fields;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_densify_apply((hipStream_t)stream_ptr, A, blocks);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_mcmc_noise(int64_t N, float *xyz, const float *opacity, const float *scaling, const float *rotation,
                   const float *z, float scale, void *stream_ptr) {
    if (N < 0 || N > 0x7fffffffLL * 256) return fail(GSR_ERR_ARG, "mcmc noise: bad N");
    if (!xyz || !opacity || !scaling || !rotation || !z) return fail(GSR_ERR_ARG, "mcmc noise: null array");
    if (!aligned16(rotation)) return fail(GSR_ERR_ARG, "mcmc noise: rotation must be 16-B aligned");
    if (N == 0) return GSR_OK;
    McmcNoise A{};
    A.N = N;
    A.xyz = xyz; A.opacity = opacity; A.scaling = scaling; A.rotation = rotation; A.z = z;
    A.scale = scale;
    const double c = 1.0 - 0.995;  // the gate's threshold on the opacity, to double precision in two floats
    A.gate_c_hi = (float)c;
    A.gate_c_lo = (float)(c - (double)A.gate_c_hi);
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_mcmc_noise((hipStream_t)stream_ptr, A);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

static void mcmc_inv_sqrt(McmcValues &V) {
    for (int k = 0; k < MCMC_MAX_RATIO; k++) V.inv_sqrt[k] = 1.0 / std::sqrt((double)(k + 1));
}

int gsr_mcmc_relocation(int64_t N, const float *opacity, const float *scaling, int activated, const int64_t *src_idx,
                        const int32_t *ratio, int64_t n, float min_opacity, float *new_opacity, float *new_scaling,
                        void *stream_ptr) {
    if (N < 0 || N > 0x7fffffffLL) return fail(GSR_ERR_ARG, "mcmc relocation: 0 <= N < 2^31");
    if (n < 0 || n > 0x7fffffffLL) return fail(GSR_ERR_ARG, "mcmc relocation: 0 <= n < 2^31");
    if (!(min_opacity > 0.f && min_opacity < 1.f)) return fail(GSR_ERR_ARG, "mcmc relocation: min_opacity must be in (0, 1)");
    if (!opacity || !scaling || !ratio || !new_opacity || !new_scaling)
        return fail(GSR_ERR_ARG, "mcmc relocation: null array");
    if (!src_idx && n > N) return fail(GSR_ERR_ARG, "mcmc relocation: n > N without src_idx");
    if (n == 0 || N == 0) return GSR_OK;
    McmcValues V{};
    V.N = N; V.n = n;
    V.opacity = opacity; V.scaling = scaling; V.src_idx = src_idx; V.ratio = ratio;
    V.new_opacity = new_opacity; V.new_scaling = new_scaling;
    V.op_stride = 1; V.sc_stride = 3;
    V.activated = activated != 0;
    V.min_opacity = min_opacity;
    mcmc_inv_sqrt(V);
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_mcmc_values((hipStream_t)stream_ptr, V);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_mcmc_apply(int64_t N, int64_t n, const int64_t *src_idx, const int64_t *dst_idx, const int32_t *occurrences,
                   float min_opacity, float *values, const gsr_densify_field *fields, int num_fields,
                   void *stream_ptr) {
    if (N < 0 || N > 0x7fffffffLL) return fail(GSR_ERR_ARG, "mcmc apply: 0 <= N < 2^31");
    if (n < 0 || n > 0x7fffffffLL) return fail(GSR_ERR_ARG, "mcmc apply: 0 <= n < 2^31");
    if (!(min_opacity > 0.f && min_opacity < 1.f)) return fail(GSR_ERR_ARG, "mcmc apply: min_opacity must be in (0, 1)");
    if (num_fields < 0 || num_fields > DENSIFY_MAX_FIELDS) return fail(GSR_ERR_ARG, "mcmc apply: 0..16 fields");
    if (!src_idx || !occurrences || !values || !fields) return fail(GSR_ERR_ARG, "mcmc apply: null input");
    const bool add = dst_idx == nullptr;
    McmcApply A{};
    A.N = N; A.n = n;
    A.src_idx = src_idx; A.dst_idx = dst_idx; A.occ = occurrences; A.values = values;
    McmcValues V{};
    int64_t blocks = 0;
    int nf = 0;
    for (int i = 0; i < num_fields; i++) {
        const gsr_densify_field &f = fields[i];
        if (f.width <= 0 || !f.dst || (add && !f.src)) return fail(GSR_ERR_ARG, "mcmc apply: field needs dst (add: src too), width > 0");
        if (f.kind < GSR_FIELD_PLAIN || f.kind > GSR_FIELD_OPACITY) return fail(GSR_ERR_ARG, "mcmc apply: bad kind");
        if ((f.kind == GSR_FIELD_OPACITY && f.width != 1) || (f.kind == GSR_FIELD_SCALING && f.width != 3))
            return fail(GSR_ERR_ARG, "mcmc apply: opacity field width must be 1, scaling field width 3");
        if (add && ((f.dst_exp_avg && !f.src_exp_avg) || (f.dst_exp_avg_sq && !f.src_exp_avg_sq)))
            return fail(GSR_ERR_ARG, "mcmc apply: moment destination without source");
        const float *cur = add ? f.src : f.dst;  // the old parameters
        if (f.kind == GSR_FIELD_OPACITY) V.opacity = cur;
        if (f.kind == GSR_FIELD_SCALING) V.scaling = cur;
        if (!add && f.kind == GSR_FIELD_STAT) continue;  // relocation leaves the statistics alone
        DensifyFieldDev &d = A.f[nf];
        d.src = f.src; d.dst = f.dst; d.src_exp_avg = f.src_exp_avg; d.src_exp_avg_sq = f.src_exp_avg_sq;
        d.dst_exp_avg = f.dst_exp_avg; d.dst_exp_avg_sq = f.dst_exp_avg_sq; d.width = f.width; d.kind = f.kind;
        A.block_start[nf++] = blocks;
        blocks += (((add ? N : 0) + n) * f.width + 255) / 256;
    }
    if (!V.opacity || !V.scaling) return fail(GSR_ERR_ARG, "mcmc apply: an opacity and a scaling field are required");
    if (blocks > 0x7fffffffLL) return fail(GSR_ERR_ARG, "mcmc apply: too many elements");
    if (N == 0 || n == 0) return GSR_OK;
    A.num_fields = nf;
    V.N = N; V.n = n;
    V.src_idx = src_idx; V.occ = occurrences;
    V.new_opacity = values; V.new_scaling = values + 1;
    V.op_stride = 4; V.sc_stride = 4;
    V.min_opacity = min_opacity;
    mcmc_inv_sqrt(V);
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_mcmc_values((hipStream_t)stream_ptr, V);
    launch_mcmc_apply((hipStream_t)stream_ptr, A, blocks);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

static int ply_setup(PlyLaunch &p, int64_t n, int record_bytes, int big_endian, const gsr_ply_column *columns,
                     int num_columns, const float *const *fields, const int *widths, int num_fields, bool pack) {
    if (n < 0 || record_bytes <= 0 || record_bytes > 48 * 1024) return fail(GSR_ERR_ARG, "ply: bad n or record size");
    if (num_columns < 0 || num_columns > PLY_MAX_COLS) return fail(GSR_ERR_ARG, "ply: at most 128 columns");
    if (num_fields < 0 || num_fields > PLY_MAX_FIELDS) return fail(GSR_ERR_ARG, "ply: at most 8 fields");
    if ((num_columns && !columns) || (num_fields && (!fields || !widths))) return fail(GSR_ERR_ARG, "ply: null table");
    int sum = 0;
    for (int f = 0; f < num_fields; f++) {
        if (widths[f] <= 0 || (n > 0 && !fields[f])) return fail(GSR_ERR_ARG, "ply: field needs width > 0 and data");
        p.field[f] = const_cast<float *>(fields[f]);
        p.width[f] = widths[f];
        sum += widths[f];
    }
    if (sum != num_columns) return fail(GSR_ERR_ARG, "ply: field widths must add up to the column count");
    static const int kSize[8] = {4, 8, 1, 1, 2, 2, 4, 4};
    for (int c = 0; c < num_columns; c++) {
        const gsr_ply_column &col = columns[c];
        if (col.type < GSR_PLY_FLOAT32 || col.type > GSR_PLY_INT32) return fail(GSR_ERR_ARG, "ply: bad column type");
        if (pack && col.type != GSR_PLY_FLOAT32) return fail(GSR_ERR_ARG, "ply: pack writes float32 columns only");
        if (col.offset < 0 || col.offset + kSize[col.type] > record_bytes)
            return fail(GSR_ERR_ARG, "ply: column outside the record");
        p.cols[c] = make_int2(col.offset, col.type);
    }
    p.n = n;
    p.record_bytes = record_bytes;
    p.rows_per_block = ply_rows_per_block(record_bytes);
    p.ncols = num_columns;
    p.nfields = num_fields;
    p.swap = big_endian ? 1 : 0;
    return GSR_OK;
}

int gsr_ply_unpack(const uint8_t *records, int64_t n, int record_bytes, int big_endian, const gsr_ply_column *columns,
                   int num_columns, float *const *fields, const int *widths, int num_fields, void *stream_ptr) {
    PlyLaunch p{};
    const int rc = ply_setup(p, n, record_bytes, big_endian, columns, num_columns, fields, widths, num_fields, false);
    if (rc != GSR_OK) return rc;
    if (n > 0 && !records) return fail(GSR_ERR_ARG, "ply: null records");
    p.records = records;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_ply((hipStream_t)stream_ptr, p, false);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_ply_pack(uint8_t *records, int64_t n, int record_bytes, int big_endian, const gsr_ply_column *columns,
                 int num_columns, const float *const *fields, const int *widths, int num_fields, void *stream_ptr) {
    PlyLaunch p{};
    const int rc = ply_setup(p, n, record_bytes, big_endian, columns, num_columns, fields, widths, num_fields, true);
    if (rc != GSR_OK) return rc;
    if (n > 0 && !records) return fail(GSR_ERR_ARG, "ply: null records");
    p.records_out = records;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_ply((hipStream_t)stream_ptr, p, true);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

size_t gsr_knn_workspace_bytes(int64_t n) { return n < 0 ? 0 : knn_workspace(n, nullptr); }

int gsr_knn_mean_dist2(int64_t n, const float *points, float *out, void *workspace, void *stream_ptr) {
    if (n < 0 || n > (int64_t)RS_ONESWEEP_MAX_N) return fail(GSR_ERR_ARG, "knn: 0 <= n < 2^30");
    if (n == 0) return GSR_OK;
    if (!points || !out || !workspace) return fail(GSR_ERR_ARG, "knn: null pointer");
    KnnScratch k{};
    k.base = workspace;
    knn_workspace(n, &k);
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_knn((hipStream_t)stream_ptr, k, points, n, out);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

// padding="valid" counts the map cropped by 5 px a side: both extents must exceed 10 (a product of two negative
// extents is positive, so the count's sign does not say this).
static bool ssim_counts_a_pixel(int H, int W, int valid_padding) { return !valid_padding || (H > 10 && W > 10); }

size_t gsr_ssim_num_partials(int planes, int H, int W) {
    return (planes > 0 && H > 0 && W > 0) ? ssim_num_partials(planes, H, W) : 0;
}

int gsr_ssim_forward(int planes, int H, int W, const float *img1, const float *img2, int valid_padding,
                     float *partial_sums, float *dm_dmu1, float *dm_dsigma1_sq, float *dm_dsigma12, void *stream_ptr) {
    if (planes <= 0 || H <= 0 || W <= 0) return fail(GSR_ERR_ARG, "ssim: empty image");
    if ((int64_t)planes * H * W > 0x7fffffffLL) return fail(GSR_ERR_ARG, "ssim: image too large");
    if (planes > 65535) return fail(GSR_ERR_ARG, "ssim: too many planes");
    if (!img1 || !img2 || !partial_sums) return fail(GSR_ERR_ARG, "ssim: null argument");
    if ((dm_dmu1 == nullptr) != (dm_dsigma1_sq == nullptr) || (dm_dmu1 == nullptr) != (dm_dsigma12 == nullptr))
        return fail(GSR_ERR_ARG, "ssim: derivative maps must be all given or all NULL");
    if (!ssim_counts_a_pixel(H, W, valid_padding))
        return fail(GSR_ERR_ARG, "ssim: image smaller than the valid window");
    hipStream_t s = (hipStream_t)stream_ptr;
    StreamDeviceGuard device_guard(s);
    launch_ssim_forward(s, planes, H, W, img1, img2, valid_padding, partial_sums, dm_dmu1, dm_dsigma1_sq, dm_dsigma12);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_ssim_backward(int planes, int H, int W, const float *img1, const float *img2, int valid_padding,
                      const float *dL_dmean, const float *dm_dmu1, const float *dm_dsigma1_sq,
                      const float *dm_dsigma12, float *dL_dimg1, void *stream_ptr) {
    if (planes <= 0 || H <= 0 || W <= 0) return fail(GSR_ERR_ARG, "ssim: empty image");
    if ((int64_t)planes * H * W > 0x7fffffffLL) return fail(GSR_ERR_ARG, "ssim: image too large");
    if (planes > 65535) return fail(GSR_ERR_ARG, "ssim: too many planes");
    if (!img1 || !img2 || !dL_dmean || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !dL_dimg1)
        return fail(GSR_ERR_ARG, "ssim: null argument");
    if (!ssim_counts_a_pixel(H, W, valid_padding))
        return fail(GSR_ERR_ARG, "ssim: image smaller than the valid window");
    const int64_t counted = (int64_t)planes * (valid_padding ? (int64_t)(H - 10) * (W - 10) : (int64_t)H * W);
    hipStream_t s = (hipStream_t)stream_ptr;
    StreamDeviceGuard device_guard(s);
    launch_ssim_backward(s, planes, H, W, img1, img2, valid_padding, dL_dmean, (float)(1.0 / (double)counted), dm_dmu1,
                         dm_dsigma1_sq, dm_dsigma12, dL_dimg1);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

// ---- bilateral grid (gsr_bilagrid.hip) ----
static const char *bilagrid_grid_error(int num, int L, int Gh, int Gw) {
    if (num <= 0 || L <= 0 || Gh <= 0 || Gw <= 0) return "bilagrid: num, L, Gh and Gw must be positive";
    if ((double)num * 12 * L * Gh * Gw > 2147483647.0)
        return "bilagrid: grid too large";
    return nullptr;
}

static const char *bilagrid_shape_error(int num, int L, int Gh, int Gw, int B, int H, int W) {
    if (const char *e = bilagrid_grid_error(num, L, Gh, Gw)) return e;
    if (B <= 0 || H <= 0 || W <= 0) return "bilagrid: B, H and W must be positive";
    if ((2 * (int64_t)std::max(H, W) + 1) * std::max(Gh, Gw) > 0x7fffffffLL || H > 16 * 65535 ||
        (int64_t)H * W > 0x7fffffffLL)
        return "bilagrid: image too large";
    return nullptr;
}

static const char *bilagrid_index_error(int num, int B, const int32_t *grid_idx) {
    if (!grid_idx) return "bilagrid: null argument";
    for (int b = 0; b < B; b++)
        if (grid_idx[b] < 0 || grid_idx[b] >= num) return "bilagrid: grid index outside [0, num)";
    return nullptr;
}

size_t gsr_bilagrid_workspace_bytes(int L, int Gh, int Gw, int H, int W) {
    if (bilagrid_shape_error(1, L, Gh, Gw, 1, H, W)) return 0;
    return bilagrid_workspace_bytes(BgShape{L, Gh, Gw, H, W});
}

int gsr_bilagrid_slice_forward(int num, int L, int Gh, int Gw, const float *grids, int B, int H, int W,
                               const float *image, const int32_t *grid_idx, float *out, void *stream_ptr) {
    if (const char *e = bilagrid_shape_error(num, L, Gh, Gw, B, H, W)) return fail(GSR_ERR_ARG, e);
    if (!grids || !image || !out) return fail(GSR_ERR_ARG, "bilagrid: null argument");
    if (const char *e = bilagrid_index_error(num, B, grid_idx)) return fail(GSR_ERR_ARG, e);
    hipStream_t s = (hipStream_t)stream_ptr;
    StreamDeviceGuard device_guard(s);
    launch_bilagrid_slice_forward(s, BgShape{L, Gh, Gw, H, W}, B, grid_idx, grids, image, out);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_bilagrid_slice_backward(int num, int L, int Gh, int Gw, const float *grids, int B, int H, int W,
                                const float *image, const int32_t *grid_idx, const float *dL_dout, float *dL_dgrids,
                                float *dL_dimage, void *workspace, void *stream_ptr) {
    if (const char *e = bilagrid_shape_error(num, L, Gh, Gw, B, H, W)) return fail(GSR_ERR_ARG, e);
    if (!grids || !image || !dL_dout) return fail(GSR_ERR_ARG, "bilagrid: null argument");
    if (const char *e = bilagrid_index_error(num, B, grid_idx)) return fail(GSR_ERR_ARG, e);
    const BgShape S{L, Gh, Gw, H, W};
    if (dL_dgrids && !workspace && bilagrid_workspace_bytes(S) > 0)
        return fail(GSR_ERR_ARG, "bilagrid: this shape needs gsr_bilagrid_workspace_bytes() of workspace");
    if (!dL_dgrids && !dL_dimage) return GSR_OK;
    hipStream_t s = (hipStream_t)stream_ptr;
    StreamDeviceGuard device_guard(s);
    if (dL_dimage) launch_bilagrid_slice_backward_image(s, S, B, grid_idx, grids, image, dL_dout, dL_dimage);
    if (dL_dgrids)
        GSR_HIP(launch_bilagrid_slice_backward_grid(s, S, num, B, grid_idx, image, dL_dout, dL_dgrids,
                                                    (float *)workspace));
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

size_t gsr_bilagrid_tv_num_partials(int num, int L, int Gh, int Gw) {
    return bilagrid_grid_error(num, L, Gh, Gw) ? 0 : bilagrid_tv_num_partials(num, L, Gh, Gw);
}

int gsr_bilagrid_tv_forward(int num, int L, int Gh, int Gw, const float *grids, float *partial_sums,
                            void *stream_ptr) {
    if (const char *e = bilagrid_grid_error(num, L, Gh, Gw)) return fail(GSR_ERR_ARG, e);
    if (!grids || !partial_sums) return fail(GSR_ERR_ARG, "bilagrid: null argument");
    hipStream_t s = (hipStream_t)stream_ptr;
    StreamDeviceGuard device_guard(s);
    launch_bilagrid_tv_forward(s, num, L, Gh, Gw, grids, partial_sums);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_bilagrid_tv_backward(int num, int L, int Gh, int Gw, const float *grids, const float *dL_dtv,
                             float *dL_dgrids, void *stream_ptr) {
    if (const char *e = bilagrid_grid_error(num, L, Gh, Gw)) return fail(GSR_ERR_ARG, e);
    if (!grids || !dL_dtv || !dL_dgrids) return fail(GSR_ERR_ARG, "bilagrid: null argument");
    hipStream_t s = (hipStream_t)stream_ptr;
    StreamDeviceGuard device_guard(s);
    launch_bilagrid_tv_backward(s, num, L, Gh, Gw, grids, dL_dtv, dL_dgrids);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

// ---- Mip-Splatting 3D smoothing filter (gsr_mipfilter.hip) ----
int gsr_mipfilter_rate(int64_t P, const float *means3D, int V, const float *cameras, float near_plane, float *rate,
                       float *zmin, int32_t *seen, void *stream_ptr) {
    if (P < 0 || P > 0x7fffffffLL * 256) return fail(GSR_ERR_ARG, "mipfilter rate: bad P");
    if (V < 1) return fail(GSR_ERR_ARG, "mipfilter rate: V must be at least 1");
    if (!std::isfinite(near_plane)) return fail(GSR_ERR_ARG, "mipfilter rate: near must be finite");
    if (!means3D || !cameras || !rate || !zmin || !seen) return fail(GSR_ERR_ARG, "mipfilter rate: null array");
    if (((uintptr_t)cameras) & 63) return fail(GSR_ERR_ARG, "mipfilter rate: the camera table must be 64-B aligned");
    if (P == 0) return GSR_OK;
    MipRateArgs A{};
    A.P = P;
    A.V = V;
    A.near = near_plane;
    A.means3D = means3D;
    A.cameras = reinterpret_cast<const MipCamera *>(cameras);
    A.rate = rate; A.zmin = zmin; A.seen = seen;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_mipfilter_rate((hipStream_t)stream_ptr, A);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_activations_filter3d_forward(int64_t N, const float *scaling, const float *opacity, const float *rotation,
                                     const float *filter_3D, float *scales, float *opacities, float *rotations,
                                     void *stream_ptr) {
    if (N < 0 || N > 0x7fffffffLL * 256) return fail(GSR_ERR_ARG, "filter3d activations: bad N");
    if (!scaling || !opacity || !rotation || !filter_3D || !scales || !opacities || !rotations)
        return fail(GSR_ERR_ARG, "filter3d activations: null array");
    if (!aligned16(rotation) || !aligned16(rotations))
        return fail(GSR_ERR_ARG, "filter3d activations: rotation arrays must be 16-B aligned");
    if (N == 0) return GSR_OK;
    Filter3DArgs A{};
    A.N = N;
    A.scaling = scaling; A.opacity = opacity; A.rotation = rotation; A.filter_3D = filter_3D;
    A.scales = scales; A.opacities = opacities; A.rotations = rotations;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_activations_filter3d_forward((hipStream_t)stream_ptr, A);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_activations_filter3d_backward(int64_t N, const float *scaling, const float *opacity, const float *rotation,
                                      const float *filter_3D, const float *dL_dscales, const float *dL_dopacities,
                                      const float *dL_drotations, float *dL_dscaling, float *dL_dopacity,
                                      float *dL_drotation, void *stream_ptr) {
    if (N < 0 || N > 0x7fffffffLL * 256) return fail(GSR_ERR_ARG, "filter3d activations: bad N");
    if (!scaling || !opacity || !rotation || !filter_3D || !dL_dscales || !dL_dopacities || !dL_drotations ||
        !dL_dscaling || !dL_dopacity || !dL_drotation)
        return fail(GSR_ERR_ARG, "filter3d activations: null array");
    if (!aligned16(rotation) || !aligned16(dL_drotations) || !aligned16(dL_drotation))
        return fail(GSR_ERR_ARG, "filter3d activations: rotation arrays must be 16-B aligned");
    if (N == 0) return GSR_OK;
    Filter3DArgs A{};
    A.N = N;
    A.scaling = scaling; A.opacity = opacity; A.rotation = rotation; A.filter_3D = filter_3D;
    A.dL_dscales = dL_dscales; A.dL_dopacities = dL_dopacities; A.dL_drotations = dL_drotations;
    A.dL_dscaling = dL_dscaling; A.dL_dopacity = dL_dopacity; A.dL_drotation = dL_drotation;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_activations_filter3d_backward((hipStream_t)stream_ptr, A);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

// ---- normal consistency (gsr_normals.hip) ----
static const char *geomfeat_error(int64_t P, const void *const *ptrs, int n, const void *const *quads, int nq) {
    if (P < 0 || P > 0x7fffffffLL * 256) return "geomfeat: bad P";
    for (int i = 0; i < n; i++)
        if (!ptrs[i]) return "geomfeat: null array";
    for (int i = 0; i < nq; i++)
        if (!aligned16(quads[i])) return "geomfeat: the (P,4) arrays must be 16-B aligned";
    return nullptr;
}

int gsr_geomfeat_forward(int64_t P, const float *means3D, const float *scales, const float *rotations,
                         const float *viewmatrix, float *out, void *stream_ptr) {
    const void *ptrs[] = {means3D, scales, rotations, viewmatrix, out}, *quads[] = {rotations, out};
    if (const char *e = geomfeat_error(P, ptrs, 5, quads, 2)) return fail(GSR_ERR_ARG, e);
    if (P == 0) return GSR_OK;
    GeomfeatArgs A{};
    A.P = P;
    A.means3D = means3D; A.scales = scales; A.rotations = rotations; A.viewmatrix = viewmatrix;
    A.out = out;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_geomfeat_forward((hipStream_t)stream_ptr, A);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_geomfeat_backward(int64_t P, const float *means3D, const float *scales, const float *rotations,
                          const float *viewmatrix, const float *dL_dout, float *dL_dmeans3D, float *dL_drotations,
                          void *stream_ptr) {
    const void *ptrs[] = {means3D, scales, rotations, viewmatrix, dL_dout, dL_dmeans3D, dL_drotations};
    const void *quads[] = {rotations, dL_dout, dL_drotations};
    if (const char *e = geomfeat_error(P, ptrs, 7, quads, 3)) return fail(GSR_ERR_ARG, e);
    if (P == 0) return GSR_OK;
    GeomfeatArgs A{};
    A.P = P;
    A.means3D = means3D; A.scales = scales; A.rotations = rotations; A.viewmatrix = viewmatrix;
    A.dL_dout = dL_dout; A.dL_dmeans3D = dL_dmeans3D; A.dL_drotations = dL_drotations;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_geomfeat_backward((hipStream_t)stream_ptr, A);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

static const char *normal_shape_error(int H, int W, float tanfovx, float tanfovy) {
    if (H <= 0 || W <= 0) return "normal consistency: H and W must be positive";
    if ((int64_t)H * W > 0x7fffffffLL || (H + 3) / 4 > 65535) return "normal consistency: image too large";
    if (!std::isfinite(tanfovx) || !std::isfinite(tanfovy) || !(tanfovx > 0.f) || !(tanfovy > 0.f))
        return "normal consistency: tanfovx and tanfovy must be finite and positive";
    return nullptr;
}

static NormalArgs normal_args(int H, int W, float tanfovx, float tanfovy) {
    NormalArgs A{};
    A.H = H; A.W = W;
    A.ifx = (float)(2.0 * (double)tanfovx / W);
    A.ify = (float)(2.0 * (double)tanfovy / H);
    A.cx = (float)(0.5 - 0.5 * W);
    A.cy = (float)(0.5 - 0.5 * H);
    return A;
}

int gsr_normal_consistency_forward(int H, int W, float tanfovx, float tanfovy, const float *D, const float *A,
                                   const float *N, float *E, float *n_d, void *stream_ptr) {
    if (const char *e = normal_shape_error(H, W, tanfovx, tanfovy)) return fail(GSR_ERR_ARG, e);
    if (!D || !A || !N || !E) return fail(GSR_ERR_ARG, "normal consistency: null array");
    NormalArgs a = normal_args(H, W, tanfovx, tanfovy);
    a.D = D; a.A = A; a.N = N; a.E = E; a.n_d = n_d;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_normal_consistency_forward((hipStream_t)stream_ptr, a);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_depth_to_normal(int H, int W, float tanfovx, float tanfovy, const float *D, const float *A, float *n_d,
                        void *stream_ptr) {
    if (const char *e = normal_shape_error(H, W, tanfovx, tanfovy)) return fail(GSR_ERR_ARG, e);
    if (!D || !A || !n_d) return fail(GSR_ERR_ARG, "normal consistency: null array");
    NormalArgs a = normal_args(H, W, tanfovx, tanfovy);
    a.D = D; a.A = A; a.n_d = n_d;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_normal_consistency_forward((hipStream_t)stream_ptr, a);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_normal_consistency_backward(int H, int W, float tanfovx, float tanfovy, const float *D, const float *A,
                                    const float *N, const float *dE, float *dD, float *dA, float *dN,
                                    void *stream_ptr) {
    if (const char *e = normal_shape_error(H, W, tanfovx, tanfovy)) return fail(GSR_ERR_ARG, e);
    if (!D || !A || !N || !dE || !dD || !dA || !dN) return fail(GSR_ERR_ARG, "normal consistency: null array");
    NormalArgs a = normal_args(H, W, tanfovx, tanfovy);
    a.D = D; a.A = A; a.N = N; a.dE = dE; a.dD = dD; a.dA = dA; a.dN = dN;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_normal_consistency_backward((hipStream_t)stream_ptr, a);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_normal_consistency_forward_surface(int H, int W, float tanfovx, float tanfovy, const float *D, const float *A,
                                           const float *N, const float *M, float depth_ratio, float *E, float *n_d,
                                           void *stream_ptr) {
    if (const char *e = normal_shape_error(H, W, tanfovx, tanfovy)) return fail(GSR_ERR_ARG, e);
    if (!D || !A || !N || !M || !E) return fail(GSR_ERR_ARG, "normal consistency: null array");
    if (!std::isfinite(depth_ratio)) return fail(GSR_ERR_ARG, "normal consistency: depth_ratio must be finite");
    NormalArgs a = normal_args(H, W, tanfovx, tanfovy);
    a.D = D; a.A = A; a.N = N; a.E = E; a.n_d = n_d; a.Md = M; a.ratio = depth_ratio;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_normal_consistency_forward((hipStream_t)stream_ptr, a);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_depth_to_normal_surface(int H, int W, float tanfovx, float tanfovy, const float *D, const float *A,
                                const float *M, float depth_ratio, float *n_d, void *stream_ptr) {
    if (const char *e = normal_shape_error(H, W, tanfovx, tanfovy)) return fail(GSR_ERR_ARG, e);
    if (!D || !A || !M || !n_d) return fail(GSR_ERR_ARG, "normal consistency: null array");
    if (!std::isfinite(depth_ratio)) return fail(GSR_ERR_ARG, "normal consistency: depth_ratio must be finite");
    NormalArgs a = normal_args(H, W, tanfovx, tanfovy);
    a.D = D; a.A = A; a.n_d = n_d; a.Md = M; a.ratio = depth_ratio;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_normal_consistency_forward((hipStream_t)stream_ptr, a);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_normal_consistency_backward_surface(int H, int W, float tanfovx, float tanfovy, const float *D, const float *A,
                                            const float *N, const float *M, float depth_ratio, const float *dE,
                                            float *dD, float *dA, float *dN, float *dM, void *stream_ptr) {
    if (const char *e = normal_shape_error(H, W, tanfovx, tanfovy)) return fail(GSR_ERR_ARG, e);
    if (!D || !A || !N || !M || !dE || !dD || !dA || !dN || !dM)
        return fail(GSR_ERR_ARG, "normal consistency: null array");
    if (!std::isfinite(depth_ratio)) return fail(GSR_ERR_ARG, "normal consistency: depth_ratio must be finite");
    NormalArgs a = normal_args(H, W, tanfovx, tanfovy);
    a.D = D; a.A = A; a.N = N; a.dE = dE; a.dD = dD; a.dA = dA; a.dN = dN; a.Md = M; a.ratio = depth_ratio; a.dM = dM;
    StreamDeviceGuard device_guard((hipStream_t)stream_ptr);
    launch_normal_consistency_backward((hipStream_t)stream_ptr, a);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_mark_visible(int P, const float *means3D, const float *viewmatrix, const float *projmatrix, uint8_t *present,
                     void *stream_ptr) {
    (void)projmatrix;
    if (P < 0) return fail(GSR_ERR_ARG, "P must be >= 0");
    if (P == 0) return GSR_OK;
    if (!means3D || !viewmatrix || !present) return fail(GSR_ERR_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream_ptr;
    StreamDeviceGuard device_guard(s);
    launch_mark_visible(s, P, means3D, viewmatrix, present);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_set_tuning(const char *name, int value) {
    const int k = find_knob(name);
    if (k < 0) return fail(GSR_ERR_ARG, std::string("gsr_set_tuning: unknown knob \"") + (name ? name : "(null)") + "\"");
    if (value != GSR_TUNING_UNSET) g_knob_value[k].store(value, std::memory_order_relaxed);
    g_knob_set[k].store(value != GSR_TUNING_UNSET, std::memory_order_relaxed);
    return GSR_OK;
}

int gsr_get_tuning(const char *name, int default_value) {
    const int k = find_knob(name);
    int v = GSR_TUNING_UNSET;
    if (k >= 0 && g_knob_set[k].load(std::memory_order_relaxed)) v = g_knob_value[k].load(std::memory_order_relaxed);
    else if (name && !strcmp(name, kStatDepthPasses)) v = g_stat_depth_passes.load(std::memory_order_relaxed);
    return v != GSR_TUNING_UNSET ? v : default_value;
}

int gsr_num_tunings(void) { return K_COUNT; }
const char *gsr_tuning_name(int i) { return (i >= 0 && i < K_COUNT) ? kKnobs[i].name : ""; }
int gsr_tuning_default(int i) { return (i >= 0 && i < K_COUNT) ? kKnobs[i].def : 0; }

int gsr_debug_wave_stamps(int which, uint32_t *host_dst, int max_slots) {
    uint4 *b = stamp_buffer(which);
    if (!b || !host_dst) return fail(GSR_ERR_ARG, "no stamp buffer");
    const int n = max_slots < STAMP_SLOTS ? max_slots : STAMP_SLOTS;
    GSR_HIP(hipDeviceSynchronize());
    GSR_HIP(hipMemcpy(host_dst, b, sizeof(uint4) * (size_t)n, hipMemcpyDeviceToHost));
    return n;
}

void gsr_set_profiling(int enable) {
    Profiler &p = prof();
    std::lock_guard<std::mutex> lk(p.mu);
    p.enabled = enable != 0;
}
int gsr_num_stages(void) { return ST_COUNT; }
const char *gsr_stage_name(int stage) { return (stage >= 0 && stage < ST_COUNT) ? kStageNames[stage] : ""; }
int gsr_stage_times(double *total_ms, int64_t *calls, int max_stages) {
    Profiler &p = prof();
    std::lock_guard<std::mutex> lk(p.mu);
    p.drain();
    const int n = max_stages < ST_COUNT ? max_stages : ST_COUNT;
    for (int i = 0; i < n; i++) {
        if (total_ms) total_ms[i] = p.total_ms[i];
        if (calls) calls[i] = p.calls[i];
    }
    return n;
}
void gsr_reset_stage_times(void) {
    Profiler &p = prof();
    std::lock_guard<std::mutex> lk(p.mu);
    p.drain();
    for (int i = 0; i < ST_COUNT; i++) {
        p.total_ms[i] = 0;
        p.calls[i] = 0;
    }
}
const char *gsr_last_error(void) { return g_err.c_str(); }
int gsr_abi_version(void) { return GSR_ABI_VERSION; }

int gsr_stream_values_supported(void) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeCanUseStreamWaitValue, dev) != hipSuccess) return 0;
    return v;
}

int gsr_stream_signal(void *stream_ptr, uint32_t *flag, uint32_t value) {
    if (!flag) return fail(GSR_ERR_ARG, "stream signal: null flag");
    hipStream_t stream = (hipStream_t)stream_ptr;
    StreamDeviceGuard device_guard(stream);
    GSR_HIP(hipStreamWriteValue32(stream, flag, value, 0));
    return GSR_OK;
}

int gsr_stream_wait(void *stream_ptr, uint32_t *flag, uint32_t value) {
    if (!flag) return fail(GSR_ERR_ARG, "stream wait: null flag");
    hipStream_t stream = (hipStream_t)stream_ptr;
    StreamDeviceGuard device_guard(stream);
    GSR_HIP(hipStreamWaitValue32(stream, flag, value, hipStreamWaitValueGte, 0xffffffffu));
    return GSR_OK;
}
const char *gsr_build_info(void) {
    return "gsrast: MI355X (gfx950) HIP rasterizer; wave64 tile compositing, LSD radix binning, "
           "deterministic gradient rows; built " __DATE__ " " __TIME__;
}

}  // extern "C"
