// lsr_api.hip -- the extern "C" boundary of liblsr.so (declared in include/lsr.h).
//
// Orchestration mirrors the reference's two native entry points (see include/lsr.h for the
// call sites they replace): forward = preprocess -> depth sort -> tile counts/scan ->
// [one D2H read of num_rendered] -> emit -> per-tile order -> render; backward = render
// replay -> per-Gaussian chain rule.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "lsr_internal.h"

using namespace lsr;

static thread_local std::string g_last_error;

// ------------------------------------------------------------------ host timeline (measurement)
// LSR_HOST_TRACE=1: host timestamps of each lsr_forward's phases, averaged and printed at exit
// (where the host spends the time between the counter hand-off and the next launches).
namespace {
struct HostTrace {
    bool on = false;
    static constexpr int kMarks = 7;
    const char* names[kMarks] = {"entry->preprocess", "->depth order", "->binning alloc", "->wait returned",
                                 "->binning enqueued", "->forward enqueued", "(unused)"};
    double acc[kMarks] = {};
    int64_t calls = 0;
    HostTrace()
    {
        const char* v = getenv("LSR_HOST_TRACE");
        on = v && v[0] == '1';
    }
    ~HostTrace()
    {
        if (!on || calls == 0) return;
        fprintf(stderr, "lsr host trace over %lld forwards (us):", (long long)calls);
        for (int i = 0; i < kMarks - 1; i++) fprintf(stderr, " %s %.2f", names[i], acc[i] / calls);
        fprintf(stderr, "\n");
    }
};
HostTrace g_host_trace;
inline double now_us()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}
struct HostMarks {
    double t[HostTrace::kMarks + 1];
    int n = 0;
    void mark()
    {
        if (g_host_trace.on && n <= HostTrace::kMarks) t[n++] = now_us();
    }
    ~HostMarks()
    {
        if (!g_host_trace.on || n < HostTrace::kMarks) return;
        for (int i = 0; i + 1 < n; i++) g_host_trace.acc[i] += t[i + 1] - t[i];
        g_host_trace.calls++;
    }
};
}  // namespace

// ------------------------------------------------------------------ opt-in event profiler
namespace {
// timing-only events: no system-scope fence (cache writeback + invalidate) when they are recorded,
// which would otherwise stall the stream around the measured launches (~6 us per step measured
// at C3 with the default flags)
constexpr unsigned kEventFlags = hipEventDisableSystemFence;
struct Pending {
    const char* name;
    hipEvent_t a, b;
};
struct Profiler {
    std::mutex mu;
    bool on = false;
    std::vector<std::string> select;  // empty: every stage
    int64_t every = 1, seen = 0;      // lsr_profile_sample: events on every `every`-th selected launch
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
    std::map<std::string, std::pair<int64_t, double>> stats;

    hipEvent_t get()
    {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, kEventFlags) != hipSuccess) return nullptr;
        return e;
    }
    void drain()
    {
        for (auto& p : pending) {
            float ms = 0.f;
            if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
                auto& st = stats[p.name];
                st.first += 1;
                st.second += ms;
            }
            pool.push_back(p.a);
            pool.push_back(p.b);
        }
        pending.clear();
    }
};
Profiler g_prof;

// Records an event pair around one launch group when profiling is on.
struct Scope {
    hipEvent_t a = nullptr, b = nullptr;
    const char* name;
    hipStream_t s;
    Scope(const char* n, hipStream_t st) : name(n), s(st)
    {
        std::lock_guard<std::mutex> g(g_prof.mu);
        if (!g_prof.on) return;
        if (!g_prof.select.empty()) {
            bool hit = false;
            for (const auto& x : g_prof.select) hit = hit || x == n;
            if (!hit) return;
        }
        if (g_prof.seen++ % g_prof.every != 0) return;
        a = g_prof.get();
        b = g_prof.get();
        if (a && b) (void)hipEventRecord(a, s);
    }
    ~Scope()
    {
        if (!a || !b) return;
        (void)hipEventRecord(b, s);
        std::lock_guard<std::mutex> g(g_prof.mu);
        g_prof.pending.push_back({name, a, b});
    }
};
}  // namespace

// ------------------------------------------------------------------ pinned host block
// Per (thread, device) pinned host memory the kernels write with system-scope stores:
//   slot[8]: the forward's one host wait -- a one-workgroup kernel publishes the counters, each with
//            the call's sequence number in one 64-bit store, and the host spins until all 8 slots
//            carry it (no pageable device-to-host copy, which is synchronous, and no
//            stream-synchronise wake-up latency);
//   stall:   set by a look-back that stopped waiting and took its fallback (lsr_debug_scan_stalls).
// Per thread, because a sequence number belongs to one caller; per device, because the block is
// written by that device's kernels.  Freed when the thread exits.
namespace {
struct HostBlock {
    uint64_t slot[8];  // {value, seq}: low word the counter, high word the sequence number
    uint32_t stall;
    uint32_t seq;      // the last sequence number used (host side)
    uint32_t bad_segment;  // lsr_decode_language_feature: a segment id outside [-N, N)
    int32_t depth_passes;  // depth-sort passes the last forward needed (0: none yet)
    // binning buffer size to request before the host wait (the last forward's, with headroom), for
    // the same P and image size; the exact size is requested after the wait if it is larger
    int32_t hint_P, hint_W, hint_H;
    size_t binning_hint;
};

struct HostBlocks {
    std::vector<std::pair<int, HostBlock*>> blocks;
    ~HostBlocks()
    {
        for (auto& b : blocks) (void)hipHostFree(b.second);
    }
    // the calling thread's block for the current device (allocated on first use); null on failure
    HostBlock* get(hipError_t* err)
    {
        int dev = 0;
        if ((*err = hipGetDevice(&dev)) != hipSuccess) return nullptr;
        for (auto& b : blocks)
            if (b.first == dev) return b.second;
        void* h = nullptr;
        if ((*err = hipHostMalloc(&h, sizeof(HostBlock), hipHostMallocCoherent)) != hipSuccess) return nullptr;
        memset(h, 0, sizeof(HostBlock));
        blocks.emplace_back(dev, static_cast<HostBlock*>(h));
        return static_cast<HostBlock*>(h);
    }
};
thread_local HostBlocks t_host;

bool counters_arrived(const HostBlock* hb, uint32_t seq)
{
    for (int i = 0; i < 8; i++)
        if ((uint32_t)(__atomic_load_n(&hb->slot[i], __ATOMIC_ACQUIRE) >> 32) != seq) return false;
    return true;
}

// Waits until the counters published with `seq` arrived; a HIP error on failure.  The stream is
// queried only after the first millisecond of waiting (then once per ~1 ms): a query costs tens of
// microseconds of host time, and counters landing during one were seen that much later.
hipError_t wait_counters(const HostBlock* hb, uint32_t seq, hipStream_t stream)
{
    if (counters_arrived(hb, seq)) return hipSuccess;
    double next_query = now_us() + 1000.0;
    for (uint64_t spin = 0;; spin++) {
        if (counters_arrived(hb, seq)) return hipSuccess;
        if ((spin & 255) == 255 && now_us() > next_query) {
            next_query = now_us() + 1000.0;
            const hipError_t q = hipStreamQuery(stream);
            if (q != hipSuccess && q != hipErrorNotReady) return q;
            if (q == hipSuccess) {  // stream idle: the stores must be visible now
                if (counters_arrived(hb, seq)) return hipSuccess;
                return hipErrorUnknown;
            }
        }
        __builtin_ia32_pause();
    }
}
}  // namespace

// who: the entry point's name where a check is shared; the text is then "<who>: <what>"
static int32_t fail(int32_t code, const char* what, hipError_t e = hipSuccess, const char* who = nullptr)
{
    char buf[512];
    const int at = who ? snprintf(buf, sizeof(buf), "%s: ", who) : 0;
    if (e != hipSuccess)
        snprintf(buf + at, sizeof(buf) - at, "%s: %s (%s)", what, hipGetErrorString(e), hipGetErrorName(e));
    else
        snprintf(buf + at, sizeof(buf) - at, "%s", what);
    g_last_error = buf;
    return code;
}

static int32_t invalid(const char* who, const char* what) { return fail(LSR_ERR_INVALID, what, hipSuccess, who); }

#define LSR_TRY(expr, what)                                                  \
    do {                                                                     \
        hipError_t _e;                                                       \
        {                                                                    \
            Scope _scope(what, stream);                                      \
            _e = (expr);                                                     \
        }                                                                    \
        if (_e == hipSuccess && debug) _e = hipStreamSynchronize(stream);    \
        if (_e == hipSuccess && debug) _e = hipGetLastError();               \
        if (_e != hipSuccess) return fail(LSR_ERR_HIP, what, _e);            \
    } while (0)

static AdamScalars adam_scalars(double lr, double beta1, double beta2, double eps, int64_t step)
{
    // torch/optim/adam.py _single_tensor_adam: Python-float scalars, cast where they meet tensors
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    AdamScalars a;
    a.w1 = (float)(1.0 - beta1);
    a.beta2 = (float)beta2;
    a.w2 = (float)(1.0 - beta2);
    a.inv_bc2_sqrt = 1.0f / (float)sqrt(bc2);
    a.eps = (float)eps;
    a.neg_step_size = (float)(-(lr / bc1));
    return a;
}

// the hyper-parameters of a device-side step (step_dev): t.step is the tensor's offset from the device count
static AdamHyper adam_hyper(const lsr_adam_tensor& t) { return AdamHyper{t.lr, t.beta1, t.beta2, t.eps, t.step}; }

// counters[kCntFwdFlags]: what a forward with these lsr_forward_flags prepared (fused_loss: it wrote the
// loss codes).  Published by the forward, and by lsr_view_restore / lsr_view_bind standing in for one.
static uint32_t forward_flags_word(int32_t flags, bool fused_loss)
{
    return ((flags & LSR_FWD_ZERO_GRAD_RECORDS) ? kFwdZeroedRecords : 0u) | (fused_loss ? kFwdFusedLoss : 0u) |
           ((flags & LSR_FWD_NO_COLOR_GRAD) ? kFwdNoColorState : 0u) | ((flags & LSR_FWD_NO_BACKWARD) ? kFwdNoBackward : 0u);
}

// The RenderParams fields every walk over a forward's lists reads, from the forward's three buffers (the
// levels gradient walk reads only the size, ranges, point_list, record and the schedule).  The caller adds
// what is its own: outputs, seeds, bind, loss, split and zero-records settings.
static RenderParams walk_params(int W, int H, const Layout& L, char* geom, char* image, char* binning)
{
    RenderParams rp{};
    rp.W = W;
    rp.H = H;
    rp.gx = L.gx;
    rp.gy = L.gy;
    rp.ranges = reinterpret_cast<const uint2*>(image + L.ranges);
    rp.point_list = reinterpret_cast<const uint32_t*>(binning + L.point_list);
    rp.cover = reinterpret_cast<uint8_t*>(binning + L.cover);
    rp.record = reinterpret_cast<const float4*>(geom + L.record);
    rp.final_T = reinterpret_cast<float*>(image + L.final_T);
    rp.n_contrib = reinterpret_cast<uint32_t*>(image + L.n_contrib);
    rp.sched_counts = reinterpret_cast<uint32_t*>(image + L.counters);
    rp.sched_lists = reinterpret_cast<uint32_t*>(image + L.tile_lists);
    rp.split_pool = reinterpret_cast<float*>(image + L.split_pool);
    rp.split_desc = reinterpret_cast<uint4*>(image + L.split_desc);
    return rp;
}

// lsr_forward_levels' additions to a forward: the extra levels' inputs and outputs, and the level
// array (LSR_BUF_LEVELS) once it is allocated
struct LevelsCall {
    int levels;  // 2 .. LSR_MAX_LEVELS
    const float* more;
    float* out_more;
    float4* lev;
};

// The gradient walk of lsr_backward_levels and lsr_levels_step_backward (A: either args struct, validated
// by its entry point; P > 0, num_rendered > 0): clears the accumulator (a->scratch) and adds every
// level's per-Gaussian sums to it; epilogue: then the accumulator -> a->dL_dlanguage_feature.
template <class A>
static int32_t levels_grad_walk(const lsr_settings* s, const A* a, hipStream_t stream, bool debug, bool epilogue)
{
    const int P = a->P, W = s->image_width, H = s->image_height, levels = a->levels;
    const Layout L = make_layout(P, W, H, a->num_rendered, 0);  // point_list sits at offset 0
    float* acc = static_cast<float*>(a->scratch);
    LSR_TRY(zero_fill(acc, sizeof(float) * 3 * (size_t)levels * (size_t)P, stream), "memset levels grad");
    LevelsGradParams gp{};
    gp.r = walk_params(W, H, L, static_cast<char*>(a->geom_buffer), static_cast<char*>(a->image_buffer),
                       static_cast<char*>(a->binning_buffer));
    gp.levels = levels;
    gp.dL_dout = a->dL_dout_language_feature;
    gp.out_lang = a->out_language_feature;
    gp.loss_gt = a->loss_target;
    gp.loss_mask = a->loss_mask;
    gp.dL_dloss = a->dL_dloss;
    gp.acc = acc;
    LSR_TRY(launch_render_levels_grad(gp, L.tiles, stream), "render levels grad");
    if (epilogue)
        LSR_TRY(launch_levels_grad_epilogue(P, levels, a->radii, acc,
                                            (a->raw & LSR_RAW_LANGUAGE) ? a->language_feature : nullptr,
                                            a->dL_dlanguage_feature, stream),
                "levels grad epilogue");
    return LSR_OK;
}

// The render forward of lsr_forward (both modes), after the binning.  lv: lsr_forward_levels' form.
static int32_t render_forward_and_finish(const lsr_settings* s, const lsr_forward_args* a, const Layout& L, char* geom,
                                         char* image, char* binning, HostBlock* hb, hipStream_t stream, bool debug,
                                         const LevelsCall* lv = nullptr)
{
    const int P = a->P, W = s->image_width, H = s->image_height;
    RenderParams rp = walk_params(W, H, L, geom, image, binning);
    rp.include_feature = (s->include_feature && a->language_feature) ? 1 : 0;
    if (a->flags & LSR_BIND_FORWARD) rp.bind = reinterpret_cast<const ViewBind*>(geom + L.view_bind);
    rp.bg = s->bg;
    rp.out_color = a->out_color;
    rp.out_lang = a->out_language_feature;
    rp.split_color = (a->flags & LSR_FWD_NO_COLOR_GRAD) ? 0 : 1;
    // a composite phase runs beside another stream's geometry phase: fewer workgroups per CU
    rp.shared_cu = (a->phase == LSR_PHASE_COMPOSITE || a->phase == LSR_PHASE_COMPOSITE_FILLED) ? 1 : 0;
    if (a->flags & LSR_FWD_NO_BACKWARD) {  // inference: no split states, no backward work lists
        rp.no_bwd = 1;
        rp.split_pool = nullptr;
    }
    if (a->flags & LSR_FWD_ZERO_GRAD_RECORDS) {
        rp.zero_records = reinterpret_cast<float4*>(geom + L.grad_records);
        rp.zero_records_n4 = ((int64_t)P * kGradStrideLang + kDeferXyOffset + 3) / 4;
    }
    if (a->out_loss && rp.include_feature) {
        rp.loss_gt = a->loss_target;
        rp.loss_mask = a->loss_mask;
        rp.loss_code = reinterpret_cast<uint8_t*>(image + L.loss_code);
        rp.loss_words = reinterpret_cast<uint64_t*>(geom + L.loss_words);
        rp.out_loss = a->out_loss;
        rp.spin_limit = stall_spin_limit();
        rp.stall = &hb->stall;
    }
    if (lv) {
        RenderLevelsParams lp{};
        lp.r = rp;
        lp.lev = lv->lev;
        lp.out_more = lv->out_more;
        lp.levels = lv->levels;
        LSR_TRY(launch_render_forward_levels(lp, L.tiles, stream), "render forward");
        return LSR_OK;
    }
    LSR_TRY(launch_render_forward(rp, L.tiles, stream), "render forward");
    return LSR_OK;
}

// The deferred language feature (lsr_forward_args.language_ready): the feature's update (another
// stream) has overlapped everything enqueued so far; the stream waits for it, then the visible
// Gaussians' records receive the feature.  Inside a graph capture the event is one recorded in the
// same capture (a join of the two branches).
static hipError_t wait_and_fill_language(const lsr_forward_args* a, const Layout& L, char* geom, hipStream_t stream)
{
    hipError_t e = hipStreamWaitEvent(stream, static_cast<hipEvent_t>(a->language_ready), 0);
    if (e != hipSuccess) return e;
    return launch_fill_language(a->P, a->language_feature, a->raw, a->radii, reinterpret_cast<float4*>(geom + L.record),
                                stream);
}

// forward_impl's argument checks (their order is part of the contract: the first fault answers); also
// clears *a->out_num_entries, before the fused-loss check
static int32_t check_forward_args(const lsr_settings* s, const lsr_forward_args* a, const LevelsCall* lv)
{
    const int P = a->P, W = s->image_width, H = s->image_height;
    if (P < 0 || W <= 0 || H <= 0 || W > 65535 * kTile || H > 65535 * kTile)
        return fail(LSR_ERR_INVALID, "lsr_forward: invalid P or image size");
    if (s->sh_degree < 0 || s->sh_degree > 3) return fail(LSR_ERR_INVALID, "lsr_forward: sh_degree must be 0..3");
    if (!a->out_color || !a->out_language_feature || (P > 0 && (!a->radii || !a->means3D || !a->opacities)))
        return fail(LSR_ERR_INVALID, "lsr_forward: missing input/output pointer");
    if (P > 0 && (!a->shs) == (!a->colors_precomp))
        return fail(LSR_ERR_INVALID, "lsr_forward: provide exactly one of shs / colors_precomp");
    if (P > 0 && ((a->scales && a->rotations) ? 1 : 0) == (a->cov3D_precomp ? 1 : 0))
        return fail(LSR_ERR_INVALID, "lsr_forward: provide exactly one of scales+rotations / cov3D_precomp");
    if (a->shs && (a->M < (s->sh_degree + 1) * (s->sh_degree + 1)))
        return fail(LSR_ERR_INVALID, "lsr_forward: M smaller than (sh_degree+1)^2");
    if (!s->bg || !s->viewmatrix || !s->projmatrix || !s->campos)
        return fail(LSR_ERR_INVALID, "lsr_forward: settings tensors missing");
    if (a->raw & ~(LSR_RAW_OPACITY | LSR_RAW_SCALES | LSR_RAW_ROTATIONS | LSR_RAW_LANGUAGE))
        return fail(LSR_ERR_INVALID, "lsr_forward: unknown raw flag");
    if (a->flags & ~(LSR_FWD_ZERO_GRAD_RECORDS | LSR_FWD_NO_COLOR_GRAD | LSR_FWD_NO_BACKWARD | LSR_BIND_FORWARD))
        return fail(LSR_ERR_INVALID, "lsr_forward: unknown flag");
    if ((a->flags & LSR_BIND_FORWARD) && (a->phase == LSR_PHASE_ALL || lv))
        return fail(LSR_ERR_INVALID, "lsr_forward: LSR_BIND_FORWARD needs a forward phase (capacity mode) of lsr_forward");
    if (a->shs_rest && (!a->shs || a->M < 2))
        return fail(LSR_ERR_INVALID, "lsr_forward: shs_rest needs shs (features_dc) and M >= 2");
    if (a->capacity_rendered < 0 || (a->capacity_rendered > 0 && a->capacity_entries <= 0) ||
        a->capacity_rendered > 0xFFFFFFFFll || a->capacity_entries > 0xFFFFFFFFll)
        return fail(LSR_ERR_INVALID, "lsr_forward: capacity mode needs capacity_rendered > 0 and capacity_entries > 0 "
                                     "(both < 2^32)");
    if (a->phase < LSR_PHASE_ALL || a->phase > LSR_PHASE_COMPOSITE_FILLED ||
        (a->phase != LSR_PHASE_ALL && (a->capacity_rendered <= 0 || a->language_ready)))
        return fail(LSR_ERR_INVALID, "lsr_forward: a forward phase needs capacity mode and no language_ready");
    if (a->out_num_entries) *a->out_num_entries = 0;
    if (a->out_loss && (!s->include_feature || (P > 0 && !a->language_feature) || !a->loss_target || !a->loss_mask))
        return fail(LSR_ERR_INVALID, "lsr_forward: the fused loss needs include_feature, language_feature, "
                                     "loss_target and loss_mask");
    return LSR_OK;
}

// P == 0: upstream leaves the images at their zero initialisation when there is nothing to draw
static int32_t forward_empty_scene(const lsr_settings* s, const lsr_forward_args* a, lsr_alloc_fn alloc, void* user,
                                   hipStream_t stream, bool debug, const LevelsCall* lv)
{
    const int W = s->image_width, H = s->image_height;
    const size_t HW = (size_t)W * H;
    LSR_TRY(zero_fill(a->out_color, 3 * HW * 4, stream), "memset color");
    LSR_TRY(zero_fill(a->out_language_feature, 3 * HW * 4, stream), "memset language");
    if (lv) LSR_TRY(zero_fill(lv->out_more, (size_t)(lv->levels - 1) * 3 * HW * 4, stream), "memset language");
    if (a->out_loss) {
        const Layout L0 = make_layout(0, W, H, 0, 0);
        char* image = static_cast<char*>(alloc(user, LSR_BUF_IMAGE, L0.image_bytes));
        if (!image) return fail(LSR_ERR_ALLOC, "lsr_forward: image buffer allocation failed");
        RenderParams rp{};
        rp.W = W;
        rp.H = H;
        rp.loss_gt = a->loss_target;
        rp.loss_mask = a->loss_mask;
        rp.loss_code = reinterpret_cast<uint8_t*>(image + L0.loss_code);
        rp.loss_partial = reinterpret_cast<double*>(image + L0.loss_partial);
        rp.out_loss = a->out_loss;
        LSR_TRY(launch_loss_background(rp, stream), "loss");
    }
    return LSR_OK;
}

// The preprocess of a forward into its geometry buffer (L: make_layout(P, W, H, 0, 0)).  The caller adds
// the placed emission's count table and the bound form's plane and table.
static PreprocessParams preprocess_params(const lsr_settings* s, const lsr_forward_args* a, const Layout& L, char* geom,
                                          uint32_t* counters)
{
    const int W = s->image_width, H = s->image_height;
    PreprocessParams pp{};
    pp.P = a->P;
    pp.M = a->M;
    pp.D = s->sh_degree;
    pp.W = W;
    pp.H = H;
    pp.gx = L.gx;
    pp.gy = L.gy;
    pp.tanfovx = s->tanfovx;
    pp.tanfovy = s->tanfovy;
    pp.focal_y = (float)H / (2.0f * s->tanfovy);
    pp.focal_x = (float)W / (2.0f * s->tanfovx);
    pp.scale_modifier = s->scale_modifier;
    pp.include_feature = s->include_feature;
    pp.prefiltered = s->prefiltered;
    pp.means = a->means3D;
    pp.shs = a->shs;
    pp.colors = a->colors_precomp;
    pp.lang = a->language_feature;
    pp.opac = a->opacities;
    pp.scales = a->scales;
    pp.rots = a->rotations;
    pp.cov_pre = a->cov3D_precomp;
    pp.view = s->viewmatrix;
    pp.proj = s->projmatrix;
    pp.campos = s->campos;
    pp.radii = a->radii;
    pp.visible = a->visible;
    pp.depth_key = reinterpret_cast<uint32_t*>(geom + L.depth_key);
    pp.tiles = reinterpret_cast<uint32_t*>(geom + L.tiles_touched);
    pp.rect = reinterpret_cast<uint32_t*>(geom + L.rect);
    pp.clamped = reinterpret_cast<uint32_t*>(geom + L.clamped);
    pp.record = reinterpret_cast<float4*>(geom + L.record);
    pp.counters = counters;
    pp.zero = reinterpret_cast<uint32_t*>(geom + L.scan_regions);
    pp.zero_words = (int)L.zero_words;  // depth-sort scan status and the fused loss's words
    pp.raw = a->raw;
    pp.shs_rest = a->shs_rest;
    pp.partial = reinterpret_cast<uint4*>(geom + L.pre_partial);
    return pp;
}

// What forward_impl's common setup hands to its three paths.
struct ForwardCall {
    const lsr_settings* s;
    const lsr_forward_args* a;
    lsr_alloc_fn alloc;
    void* user;
    hipStream_t stream;
    bool debug;
    int64_t* num_rendered;
    LevelsCall* lv;
    Layout L;  // make_layout(P, W, H, 0, 0): the geometry and image buffers' (each path sizes its binning)
    HostBlock* hb;
    char *geom, *image;
    uint32_t* counters;
    bool placed;    // placed emission (the MSD depth order's fused emission at super-tile-major positions)
    bool deferred;  // geometry first, the language feature after the caller's event or in the composite call
};

// capacity mode's entry capacity: the MSD depth order's fused emission holds at most L.fused_cap entries
static int64_t entry_capacity(const lsr_forward_args* a, const Layout& L)
{
    return !depth_order_uses_pass_count(a->P) ? std::min<int64_t>(a->capacity_entries, L.fused_cap) : a->capacity_entries;
}

// LSR_PHASE_COMPOSITE / LSR_PHASE_COMPOSITE_FILLED: the geometry call's buffers (same allocator keys and
// sizes): the feature (unless a fused update already wrote it, LSR_PHASE_COMPOSITE_FILLED), then the
// compositing
static int32_t forward_composite(const ForwardCall& f)
{
    const lsr_forward_args* a = f.a;
    hipStream_t stream = f.stream;
    const bool debug = f.debug, bound = (a->flags & LSR_BIND_FORWARD) != 0;
    const int P = a->P;
    const int64_t R_cap = a->capacity_rendered;
    const Layout L = make_layout(P, f.s->image_width, f.s->image_height, R_cap, entry_capacity(a, f.L));
    char* binning = static_cast<char*>(f.alloc(f.user, LSR_BUF_BINNING, L.binning_bytes));
    if (!binning) return fail(LSR_ERR_ALLOC, "lsr_forward: binning buffer allocation failed");
    *f.num_rendered = R_cap;
    if (f.deferred && a->phase == LSR_PHASE_COMPOSITE) {
        LSR_TRY(launch_fill_language(P, a->language_feature, a->raw, a->radii,
                                     reinterpret_cast<float4*>(f.geom + (bound ? L.lang_plane : L.record)), stream,
                                     bound ? 1 : 0),
                "fill language");
        if (f.lv)
            LSR_TRY(launch_fill_levels(P, f.lv->levels, f.lv->more, a->raw, a->radii, f.lv->lev, stream), "fill levels");
    }
    return render_forward_and_finish(f.s, a, L, f.geom, f.image, binning, f.hb, stream, debug, f.lv);
}

// Capacity mode, after the preprocess: nothing waits for the device.  The counters stay on the device, the
// binning's grids and buffers come from the capacities and its kernels read the true counts; a view over
// capacity sets counters[kCntOverflow] (and *overflow) and is not binned.  binning: the bound form's,
// taken before the preprocess, else null.
static int32_t forward_capacity(const ForwardCall& f, uint4* partial, uint32_t fwd_flags, char* binning)
{
    const lsr_forward_args* a = f.a;
    hipStream_t stream = f.stream;
    const bool debug = f.debug;
    HostBlock* hb = f.hb;
    const int P = a->P;
    const int64_t R_cap = a->capacity_rendered;
    const bool fused = !depth_order_uses_pass_count(P);
    const int64_t E_cap = entry_capacity(a, f.L);
    // LSD order (large P): the passes this thread's last eager forward needed (its key range is
    // not read on the host here; a view that needs more is flagged as over capacity)
    const int passes = fused ? 0 : (hb->depth_passes > 0 ? hb->depth_passes : 4);
    LSR_TRY(launch_publish_counters((P + kPreThreads - 1) / kPreThreads, partial, f.counters, nullptr, 0, fwd_flags,
                                    (uint32_t)R_cap, (uint32_t)E_cap, a->overflow, passes, stream),
            "publish counters");
    LSR_TRY(launch_depth_order(P, fused ? 4 : passes, f.L, f.geom, f.counters, &hb->stall, stream, debug, fused,
                               (uint32_t)E_cap, f.placed),
            "depth order");
    const Layout L = make_layout(P, f.s->image_width, f.s->image_height, R_cap, E_cap);
    if (!binning) binning = static_cast<char*>(f.alloc(f.user, LSR_BUF_BINNING, L.binning_bytes));
    if (!binning) return fail(LSR_ERR_ALLOC, "lsr_forward: binning buffer allocation failed");
    LSR_TRY(launch_binning(P, R_cap, L, f.geom, f.image, binning, &hb->stall, stream, debug, fused,
                           DevCount{f.counters + kCntSuper, f.counters + kCntOverflow}, f.placed),
            "binning");
    *f.num_rendered = R_cap;
    if (a->phase == LSR_PHASE_GEOMETRY) return LSR_OK;
    if (f.deferred) LSR_TRY(wait_and_fill_language(a, L, f.geom, stream), "fill language");
    // (lsr_levels_step_forward, one phase: level 0 went into the records in the preprocess)
    if (f.lv) LSR_TRY(launch_fill_levels(P, f.lv->levels, f.lv->more, a->raw, a->radii, f.lv->lev, stream), "fill levels");
    return render_forward_and_finish(f.s, a, L, f.geom, f.image, binning, hb, stream, debug, f.lv);
}

// The eager forward, after the preprocess, with the one host wait: num_rendered R and the super-tile
// entries E size the binning buffer, and the visible depth-key range fixes the number of depth-sort
// passes.  The depth sort is enqueued BEFORE the wait, with this thread's last pass count: it reads the
// key range on the device, and any pass count >= the needed one gives the same order (the extra digits are
// all 0), so the GPU sorts while the host waits, instead of idling until the host has enqueued the next
// launch.  Should the range need more passes than guessed, the sort is run again below.
static int32_t forward_eager(const ForwardCall& f, uint4* partial, uint32_t fwd_flags, HostMarks& hm)
{
    const lsr_settings* s = f.s;
    const lsr_forward_args* a = f.a;
    hipStream_t stream = f.stream;
    const bool debug = f.debug, placed = f.placed;
    HostBlock* hb = f.hb;
    LevelsCall* lv = f.lv;
    char *geom = f.geom, *image = f.image;
    uint32_t* counters = f.counters;
    const int P = a->P, W = s->image_width, H = s->image_height;
    const uint32_t seq = ++hb->seq == 0 ? ++hb->seq : hb->seq;
    LSR_TRY(launch_publish_counters((P + kPreThreads - 1) / kPreThreads, partial, counters, hb->slot, seq, fwd_flags, 0u,
                                    0u, nullptr, 0, stream),
            "publish counters");
    const int guess = hb->depth_passes > 0 ? hb->depth_passes : 4;
    // MSD path: the bucket sort also emits the super-tile entries (into geometry arrays of fixed
    // capacity, so no host value is needed); used below when they fitted
    const bool fused_emit = !depth_order_uses_pass_count(P);
    LSR_TRY(launch_depth_order(P, guess, f.L, geom, counters, &hb->stall, stream, debug, fused_emit, 0, placed),
            "depth order");
    // the extra levels' features of the visible Gaussians (radii are the preprocess's): enqueued here,
    // so it runs while the host waits for the counts
    if (lv) LSR_TRY(launch_fill_levels(P, lv->levels, lv->more, a->raw, a->radii, lv->lev, stream), "fill levels");
    hm.mark();
    // the binning buffer from the last forward's size while the GPU works (the allocator callback
    // is host work that would otherwise sit between the wait and the binning launches)
    char* binning = nullptr;
    size_t binning_have = 0;
    if (hb->binning_hint && hb->hint_P == P && hb->hint_W == W && hb->hint_H == H) {
        binning = static_cast<char*>(f.alloc(f.user, LSR_BUF_BINNING, hb->binning_hint));
        binning_have = binning ? hb->binning_hint : 0;
    }
    hm.mark();
    LSR_TRY(wait_counters(hb, seq, stream), "wait counters");
    hm.mark();
    uint32_t host_cnt[8];
    for (int i = 0; i < 8; i++) host_cnt[i] = (uint32_t)hb->slot[i];
    if (host_cnt[kCntError] && s->prefiltered)
        return fail(LSR_ERR_PREFILTERED, "lsr_forward: prefiltered=True but a Gaussian is outside the frustum");
    const int64_t R = host_cnt[kCntRendered];
    *f.num_rendered = R;
    if (a->out_num_entries) *a->out_num_entries = (int64_t)host_cnt[kCntSuper];
    if (R > 0) {
        // sort only the bits the visible keys span (key - min <= max - min)
        const uint32_t span = host_cnt[kCntKeyMax] - host_cnt[kCntKeyMin];
        int bits = 0;
        while (bits < 32 && (span >> bits) != 0) bits++;
        const int passes = bits <= 8 ? 1 : (bits + 7) / 8;
        if (depth_order_uses_pass_count(P)) hb->depth_passes = passes;
        if (depth_order_uses_pass_count(P) && passes > guess) {  // short guess: clear the scan status, sort again
            LSR_TRY(zero_fill(geom + f.L.scan_regions, 4 * kDepthScans * f.L.scan_region_geom, stream),
                    "clear scan status");
            LSR_TRY(launch_depth_order(P, passes, f.L, geom, counters, &hb->stall, stream, debug), "depth order");
        }
    }

    const bool emitted = fused_emit && (int64_t)host_cnt[kCntSuper] <= f.L.fused_cap;
    if (fused_emit && !emitted) {  // entries beyond the fused capacity: the depth order again, unfused
        LSR_TRY(zero_fill(geom + f.L.scan_regions, 4 * f.L.zero_words, stream), "clear scan status");
        LSR_TRY(launch_depth_order(P, guess, f.L, geom, counters, &hb->stall, stream, debug, false), "depth order");
    }
    const Layout L = make_layout(P, W, H, R, (int64_t)host_cnt[kCntSuper]);
    if (!binning || L.binning_bytes > binning_have) {
        binning = static_cast<char*>(f.alloc(f.user, LSR_BUF_BINNING, L.binning_bytes));
        if (!binning) return fail(LSR_ERR_ALLOC, "lsr_forward: binning buffer allocation failed");
    }
    hb->hint_P = P;
    hb->hint_W = W;
    hb->hint_H = H;
    hb->binning_hint = L.binning_bytes + L.binning_bytes / 8;  // 12.5 % headroom for the next view
    LSR_TRY(launch_binning(P, R, L, geom, image, binning, &hb->stall, stream, debug, emitted, DevCount{nullptr, nullptr},
                           placed),
            "binning");
    if (f.deferred) LSR_TRY(wait_and_fill_language(a, L, geom, stream), "fill language");
    hm.mark();
    const int32_t rc = render_forward_and_finish(s, a, L, geom, image, binning, hb, stream, debug, lv);
    hm.mark();
    return rc;
}

// lsr_forward, and with lv lsr_forward_levels (validated there: inference, one phase, no capacity
// mode, no fused loss, no deferred feature) or lsr_levels_step_forward (capacity mode; all phases but
// the geometry one).
static int32_t forward_impl(const lsr_settings* s, const lsr_forward_args* a, lsr_alloc_fn alloc, void* user,
                            void* stream_ptr, int64_t* num_rendered, LevelsCall* lv)
{
    if (!s || !a || !alloc || !num_rendered) return fail(LSR_ERR_INVALID, "lsr_forward: null argument");
    if (const int32_t rc = check_forward_args(s, a, lv)) return rc;
    const int P = a->P, W = s->image_width, H = s->image_height;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = s->debug != 0;
    *num_rendered = 0;
    if (P == 0) return forward_empty_scene(s, a, alloc, user, stream, debug, lv);

    HostMarks hm;
    hm.mark();
    ForwardCall f{s, a, alloc, user, stream, debug, num_rendered, lv, make_layout(P, W, H, 0, 0)};
    const Layout& L = f.L;
    if (L.supers > 65536) return fail(LSR_ERR_INVALID, "lsr_forward: image larger than 65536 super-tiles");
    hipError_t herr = hipSuccess;
    f.hb = t_host.get(&herr);
    if (!f.hb) return fail(LSR_ERR_HIP, "lsr_forward: pinned host block", herr);
    char* geom = f.geom = static_cast<char*>(alloc(user, LSR_BUF_GEOM, L.geom_bytes));
    f.image = static_cast<char*>(alloc(user, LSR_BUF_IMAGE, L.image_bytes));
    if (!f.geom || !f.image) return fail(LSR_ERR_ALLOC, "lsr_forward: geometry/image buffer allocation failed");
    if (lv) {
        lv->lev = static_cast<float4*>(alloc(user, LSR_BUF_LEVELS, lsr_levels_bytes(P, lv->levels)));
        if (!lv->lev) return fail(LSR_ERR_ALLOC, "lsr_forward_levels: level buffer allocation failed");
    }
    // no memset: k_publish_counters initialises every counter word before anything reads it
    f.counters = reinterpret_cast<uint32_t*>(f.image + L.counters);
    f.placed = !depth_order_uses_pass_count(P) && placed_emit(L, a->phase == LSR_PHASE_GEOMETRY, msd_digits(P));
    f.deferred = (a->language_ready || a->phase != LSR_PHASE_ALL) && s->include_feature && a->language_feature;
    if (a->phase == LSR_PHASE_COMPOSITE || a->phase == LSR_PHASE_COMPOSITE_FILLED) return forward_composite(f);

    PreprocessParams pp = preprocess_params(s, a, L, geom, f.counters);
    if (f.placed) {  // the bucket sort's count table
        pp.zero2 = reinterpret_cast<uint32_t*>(geom + L.sup_status);
        pp.zero2_words = (int)sup_words(msd_digits(P));
    }
    pp.lang_deferred = f.deferred ? 1 : 0;
    // the bound form's geometry phase (a cache miss): b into the plane and the identity table by the
    // preprocess, which needs the point list's address: the binning buffer is taken first
    char* bound_binning = nullptr;
    if (a->flags & LSR_BIND_FORWARD) {
        const Layout Lc = make_layout(P, W, H, a->capacity_rendered, entry_capacity(a, L));
        bound_binning = static_cast<char*>(alloc(user, LSR_BUF_BINNING, Lc.binning_bytes));
        if (!bound_binning) return fail(LSR_ERR_ALLOC, "lsr_forward: binning buffer allocation failed");
        pp.plane = reinterpret_cast<float4*>(geom + L.lang_plane);
        pp.bind = reinterpret_cast<ViewBind*>(geom + L.view_bind);
        pp.bind_point_list = reinterpret_cast<const uint32_t*>(bound_binning + Lc.point_list);
    }
    LSR_TRY(launch_preprocess(pp, stream), "preprocess");
    hm.mark();
    const uint32_t fwd_flags = forward_flags_word(a->flags, a->out_loss && s->include_feature && a->language_feature);
    if (a->capacity_rendered > 0) return forward_capacity(f, pp.partial, fwd_flags, bound_binning);
    return forward_eager(f, pp.partial, fwd_flags, hm);
}

// lsr_forward_levels and lsr_levels_step_forward (who) after their null check: the checks they share, in
// the order both make them, and the forward.  The entry point's own checks (fwd.phase and the capacity
// fields) sit between the shared ones: own(a) makes them, 0 when they pass.  reserved: a reserved field of
// its args is set; flags_text: its wording of the fwd.flags refusal.
template <class Own>
static int32_t forward_levels(const char* who, const lsr_settings* s, const lsr_forward_levels_args* la, bool reserved,
                              const char* flags_text, Own own, lsr_alloc_fn alloc, void* user, void* stream_ptr,
                              int64_t* num_rendered)
{
    const lsr_forward_args* a = &la->fwd;
    if (la->levels < 1 || la->levels > LSR_MAX_LEVELS) return invalid(who, "levels must be 1..LSR_MAX_LEVELS (4)");
    if (reserved) return invalid(who, "reserved must be 0");
    if (!s->include_feature) return invalid(who, "needs settings.include_feature");
    if (a->flags != LSR_FWD_NO_BACKWARD) return invalid(who, flags_text);
    if (a->loss_target) return invalid(who, "no fused loss, fwd.loss_target must be NULL");
    if (a->loss_mask) return invalid(who, "no fused loss, fwd.loss_mask must be NULL");
    if (a->out_loss) return invalid(who, "no fused loss, fwd.out_loss must be NULL");
    if (a->language_ready) return invalid(who, "fwd.language_ready must be NULL");
    if (const int32_t rc = own(a)) return rc;
    if (a->P > 0 && !a->language_feature) return invalid(who, "fwd.language_feature (level 0) is NULL");
    if (la->levels > 1 && a->P > 0 && !la->more_language_feature)
        return invalid(who, "more_language_feature is NULL with levels > 1");
    if (la->levels > 1 && !la->more_out_language_feature)
        return invalid(who, "more_out_language_feature is NULL with levels > 1");
    if (la->levels == 1) return forward_impl(s, a, alloc, user, stream_ptr, num_rendered, nullptr);
    LevelsCall lv{la->levels, la->more_language_feature, la->more_out_language_feature, nullptr};
    return forward_impl(s, a, alloc, user, stream_ptr, num_rendered, &lv);
}

// The checks of lsr_backward_levels and lsr_levels_step_backward (who; A: its args struct, whose fields
// of these names mean the same).  The step form has a second reserved field, takes num_rendered as the
// forward's capacity (never 0) and may leave dL_dlanguage_feature NULL with update.
template <class A>
static int32_t check_levels_backward(const char* who, const lsr_settings* s, const A* a)
{
    constexpr bool step = std::is_same<A, lsr_levels_step_backward_args>::value;
    if (!s) return invalid(who, "settings is NULL");
    if (!a) return invalid(who, "args is NULL");
    if (a->levels < 1 || a->levels > LSR_MAX_LEVELS) return invalid(who, "levels must be 1..LSR_MAX_LEVELS (4)");
    bool reserved = a->reserved != 0;
    if constexpr (step) reserved = reserved || a->reserved2 != 0;
    if (reserved) return invalid(who, "reserved must be 0");
    if (a->P < 0) return invalid(who, "P must not be negative");
    if (a->num_rendered < 0) return invalid(who, "num_rendered must not be negative");
    if (!s->include_feature) return invalid(who, "needs settings.include_feature");
    if (s->image_width <= 0 || s->image_height <= 0) return invalid(who, "invalid settings.image_width / image_height");
    if (a->P > 0) {
        if constexpr (step) {
            if (a->num_rendered == 0) return invalid(who, "num_rendered is the forward's capacity, > 0");
        }
        if (!a->geom_buffer) return invalid(who, "geom_buffer is NULL");
        if (!a->binning_buffer) return invalid(who, "binning_buffer is NULL");
        if (!a->image_buffer) return invalid(who, "image_buffer is NULL");
        if (!a->radii) return invalid(who, "radii is NULL");
        if (!a->scratch) return invalid(who, "scratch is NULL");
        if constexpr (step) {
            if (!a->dL_dlanguage_feature && !a->update) return invalid(who, "dL_dlanguage_feature is NULL without update");
        } else {
            if (!a->dL_dlanguage_feature) return invalid(who, "dL_dlanguage_feature is NULL");
        }
        if ((a->raw & LSR_RAW_LANGUAGE) && !a->language_feature)
            return invalid(who, "language_feature is NULL with raw & LSR_RAW_LANGUAGE");
    }
    const int fused = (a->out_language_feature ? 1 : 0) + (a->loss_target ? 1 : 0) + (a->loss_mask ? 1 : 0) +
                      (a->dL_dloss ? 1 : 0);
    if (fused != 0 && fused != 4)
        return invalid(who, "the fused seed needs out_language_feature, loss_target, loss_mask and dL_dloss, all four "
                            "or none");
    if (fused == 0 && !a->dL_dout_language_feature)
        return invalid(who, "no seed, give dL_dout_language_feature or the fused seed (dL_dloss)");
    return LSR_OK;
}

extern "C" {

int32_t lsr_abi_version(void) { return LSR_ABI_VERSION; }

const char* lsr_last_error(void) { return g_last_error.c_str(); }

size_t lsr_geom_bytes(int32_t P, int32_t width, int32_t height) { return make_layout(P, width, height, 0, 0).geom_bytes; }

size_t lsr_image_bytes(int32_t width, int32_t height) { return make_layout(0, width, height, 0, 0).image_bytes; }

// every super-tile entry carries at least one tile instance, so E <= num_rendered
size_t lsr_binning_bytes(int32_t width, int32_t height, int64_t num_rendered)
{
    return make_layout(0, width, height, num_rendered, num_rendered).binning_bytes;
}

size_t lsr_backward_bytes(int32_t P) { return 4 * (size_t)kGradStride * (size_t)(P > 0 ? P : 1); }

int32_t lsr_state_layout_of(int32_t P, int32_t width, int32_t height, int64_t num_rendered, lsr_state_layout* out)
{
    if (!out || P < 0 || width < 0 || height < 0 || num_rendered < 0)
        return fail(LSR_ERR_INVALID, "lsr_state_layout_of: invalid argument");
    const Layout L = make_layout(P, width, height, num_rendered, 0);
    out->depth_key = L.depth_key;
    out->tiles_touched = L.tiles_touched;
    out->rect = L.rect;
    out->record = L.record;
    out->clamped = L.clamped;
    out->sorted_ids = L.sorted_ids;
    out->super_offset = L.super_offset;
    out->counters = L.counters;
    out->ranges = L.ranges;
    out->final_T = L.final_T;
    out->n_contrib = L.n_contrib;
    out->point_list = L.point_list;
    out->grad_records = L.grad_records;
    return LSR_OK;
}

int32_t lsr_forward(const lsr_settings* s, const lsr_forward_args* a, lsr_alloc_fn alloc, void* user,
                    void* stream_ptr, int64_t* num_rendered)
{
    return forward_impl(s, a, alloc, user, stream_ptr, num_rendered, nullptr);
}

int32_t lsr_debug_levels_occupancy(int32_t levels)
{
    if (levels < 1 || levels > LSR_MAX_LEVELS)
        return -fail(LSR_ERR_INVALID, "lsr_debug_levels_occupancy: levels must be 1..LSR_MAX_LEVELS (4)");
    const int n = render_forward_occupancy(levels);
    return n >= 0 ? n : -fail(LSR_ERR_HIP, "lsr_debug_levels_occupancy: occupancy query failed");
}

size_t lsr_levels_bytes(int32_t P, int32_t levels)
{
    if (P <= 0 || levels < 2 || levels > LSR_MAX_LEVELS) return 0;
    return align_up(sizeof(float4) * (size_t)level_quads(levels) * (size_t)P);
}

int32_t lsr_forward_levels(const lsr_settings* s, const lsr_forward_levels_args* la, lsr_alloc_fn alloc, void* user,
                           void* stream_ptr, int64_t* num_rendered)
{
    static const char who[] = "lsr_forward_levels";
    if (!s || !la || !alloc || !num_rendered) return invalid(who, "null argument");
    const auto own = [](const lsr_forward_args* a) {
        if (a->phase != LSR_PHASE_ALL) return invalid(who, "fwd.phase must be LSR_PHASE_ALL");
        if (a->capacity_rendered != 0) return invalid(who, "no capacity mode, fwd.capacity_rendered must be 0");
        return (int32_t)LSR_OK;
    };
    return forward_levels(who, s, la, la->reserved != 0, "inference only, fwd.flags must be LSR_FWD_NO_BACKWARD", own,
                          alloc, user, stream_ptr, num_rendered);
}

size_t lsr_backward_levels_bytes(int32_t P, int32_t levels)
{
    if (P <= 0 || levels < 1 || levels > LSR_MAX_LEVELS) return 0;
    return align_up(sizeof(float) * 3 * (size_t)levels * (size_t)P);
}

int32_t lsr_backward_levels(const lsr_settings* s, const lsr_backward_levels_args* a, void* stream_ptr)
{
    if (const int32_t rc = check_levels_backward("lsr_backward_levels", s, a)) return rc;
    const int P = a->P, levels = a->levels;
    if (P == 0) return LSR_OK;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = s->debug != 0;
    if (a->num_rendered == 0) {  // nothing was drawn: no Gaussian has a weight in any pixel
        LSR_TRY(zero_fill(a->dL_dlanguage_feature, sizeof(float) * 3 * (size_t)levels * (size_t)P, stream),
                "memset dlang levels");
        return LSR_OK;
    }
    return levels_grad_walk(s, a, stream, debug, true);
}

int32_t lsr_levels_step_forward(const lsr_settings* s, const lsr_levels_step_forward_args* sa, lsr_alloc_fn alloc,
                                void* user, void* stream_ptr, int64_t* num_rendered)
{
    static const char who[] = "lsr_levels_step_forward";
    if (!s || !sa || !alloc || !num_rendered) return invalid(who, "null argument");
    const lsr_forward_levels_args* la = &sa->levels;
    const auto own = [](const lsr_forward_args* a) {
        if (a->capacity_rendered <= 0) return invalid(who, "capacity mode only, fwd.capacity_rendered must be > 0");
        if (a->capacity_entries <= 0) return invalid(who, "capacity mode only, fwd.capacity_entries must be > 0");
        if (!a->overflow) return invalid(who, "capacity mode only, fwd.overflow is NULL");
        if (a->phase == LSR_PHASE_GEOMETRY)
            return invalid(who, "fwd.phase LSR_PHASE_GEOMETRY is lsr_forward's (the geometry does not depend on the "
                                "levels): call lsr_forward with that phase");
        if (a->phase != LSR_PHASE_ALL && a->phase != LSR_PHASE_COMPOSITE && a->phase != LSR_PHASE_COMPOSITE_FILLED)
            return invalid(who, "fwd.phase must be LSR_PHASE_ALL, LSR_PHASE_COMPOSITE or LSR_PHASE_COMPOSITE_FILLED");
        return (int32_t)LSR_OK;
    };
    return forward_levels(who, s, la, sa->reserved != 0 || la->reserved != 0,
                          "fwd.flags must be LSR_FWD_NO_BACKWARD (the gradient walk needs no backward state)", own, alloc,
                          user, stream_ptr, num_rendered);
}

int32_t lsr_levels_step_backward(const lsr_settings* s, const lsr_levels_step_backward_args* a, void* stream_ptr)
{
    if (const int32_t rc = check_levels_backward("lsr_levels_step_backward", s, a)) return rc;
    const int P = a->P, levels = a->levels;
    if (a->update) {
        const lsr_adam_tensor& u = *a->update;
        if (!(a->raw & LSR_RAW_LANGUAGE))
            return fail(LSR_ERR_INVALID, "lsr_levels_step_backward: update needs raw & LSR_RAW_LANGUAGE (the raw "
                                         "features are what Adam steps)");
        if (u.param != a->language_feature)
            return fail(LSR_ERR_INVALID, "lsr_levels_step_backward: update->param must be language_feature");
        if (u.n != 3 * (int64_t)levels * (int64_t)P)
            return fail(LSR_ERR_INVALID, "lsr_levels_step_backward: update->n must be 3 * levels * P");
        if (P > 0 && (!u.exp_avg || !u.exp_avg_sq))
            return fail(LSR_ERR_INVALID, "lsr_levels_step_backward: update->exp_avg / exp_avg_sq is NULL");
        if (!a->update_step_dev) return fail(LSR_ERR_INVALID, "lsr_levels_step_backward: update_step_dev is NULL");
        if (a->fill_record && levels > 1 && !a->fill_levels)
            return fail(LSR_ERR_INVALID, "lsr_levels_step_backward: fill_levels is NULL with levels > 1 and fill_record");
        if (a->fill_levels && !a->fill_record)
            return fail(LSR_ERR_INVALID, "lsr_levels_step_backward: fill_levels needs fill_record");
    } else if (a->update_step_dev || a->update_skip || a->fill_record || a->fill_levels) {
        return fail(LSR_ERR_INVALID, "lsr_levels_step_backward: update_step_dev / update_skip / fill_record / "
                                     "fill_levels need update");
    }
    if (P == 0) return LSR_OK;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = s->debug != 0;
    // no early return for an empty view: num_rendered is the capacity.  A view that drew nothing, or
    // one over capacity, left empty ranges and no scheduled tile: the walk's workgroups all return
    if (const int32_t rc = levels_grad_walk(s, a, stream, debug, !a->update)) return rc;
    if (!a->update) return LSR_OK;
    const lsr_adam_tensor& u = *a->update;
    LSR_TRY(launch_levels_tail(P, levels, a->radii, static_cast<float*>(a->scratch), u.param, u.exp_avg, u.exp_avg_sq, a->dL_dlanguage_feature,
                               adam_hyper(u), a->update_step_dev, a->update_skip, reinterpret_cast<float4*>(a->fill_record),
                               static_cast<float4*>(a->fill_levels), stream),
            "levels tail");
    return LSR_OK;
}

int32_t lsr_backward(const lsr_settings* s, const lsr_backward_args* a, lsr_alloc_fn alloc, void* user,
                     void* stream_ptr)
{
    if (!s || !a || !alloc) return fail(LSR_ERR_INVALID, "lsr_backward: null argument");
    const int P = a->P, W = s->image_width, H = s->image_height;
    if (P < 0 || W <= 0 || H <= 0) return fail(LSR_ERR_INVALID, "lsr_backward: invalid P or image size");
    // geometry outputs: all given (full backward) or all NULL (screen-space + language only)
    const bool geometry = a->dL_dcolors || a->dL_dopacity || a->dL_dmeans3D || a->dL_dcov3D || a->dL_dsh ||
                          a->dL_dsh_rest || a->dL_dscales || a->dL_drotations;
    if (geometry) {
        if (!a->dL_dmeans2D || !a->dL_dcolors || !a->dL_dlanguage_feature || !a->dL_dopacity || !a->dL_dmeans3D)
            return fail(LSR_ERR_INVALID, "lsr_backward: missing output pointer");
        if ((a->shs && !a->dL_dsh) || (a->cov3D_precomp && !a->dL_dcov3D))
            return fail(LSR_ERR_INVALID, "lsr_backward: missing dL_dsh / dL_dcov3D output");
    }
    if (a->raw & ~(LSR_RAW_OPACITY | LSR_RAW_SCALES | LSR_RAW_ROTATIONS | LSR_RAW_LANGUAGE))
        return fail(LSR_ERR_INVALID, "lsr_backward: unknown raw flag");
    if (a->flags & ~(LSR_BWD_RECORDS_ZEROED | LSR_BWD_SHARED_CU | LSR_BWD_DEFER_TAIL | LSR_BIND_BACKWARD |
                     LSR_BIND_FILL_PLANE))
        return fail(LSR_ERR_INVALID, "lsr_backward: unknown flag");
    if ((a->flags & LSR_BIND_FILL_PLANE) && !a->fill_record)
        return fail(LSR_ERR_INVALID, "lsr_backward: LSR_BIND_FILL_PLANE needs fill_record (the plane)");
    const bool defer = (a->flags & LSR_BWD_DEFER_TAIL) != 0;
    if (defer && !a->update) return fail(LSR_ERR_INVALID, "lsr_backward: LSR_BWD_DEFER_TAIL needs update");
    if (geometry && a->shs_rest && (!a->shs || a->M < 2 || !a->dL_dsh_rest))
        return fail(LSR_ERR_INVALID, "lsr_backward: shs_rest needs shs, M >= 2 and dL_dsh_rest");
    if ((a->raw & LSR_RAW_OPACITY) && P > 0 && !a->opacities)
        return fail(LSR_ERR_INVALID, "lsr_backward: raw opacities missing");
    if (a->update) {
        const lsr_adam_tensor& u = *a->update;
        if (geometry || a->dL_dout_color || !(a->raw & LSR_RAW_LANGUAGE) || !s->include_feature || !a->language_feature ||
            u.param != a->language_feature || u.n != 3 * (int64_t)P || !u.exp_avg || !u.exp_avg_sq ||
            !a->update_step_dev || !a->dL_dlanguage_feature)
            return fail(LSR_ERR_INVALID, "lsr_backward: a fused update needs the language-only backward of the raw "
                                         "language feature (update->param), its moments, a step block and "
                                         "dL_dlanguage_feature");
    } else if (a->fill_record || a->update_step_dev || a->update_skip) {
        return fail(LSR_ERR_INVALID, "lsr_backward: fill_record / update_step_dev / update_skip need update");
    }
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = s->debug != 0;
    if (P == 0) return LSR_OK;
    if (!a->geom_buffer || !a->image_buffer || !a->binning_buffer || !a->radii)
        return fail(LSR_ERR_INVALID, "lsr_backward: missing forward state");
    const Layout L = make_layout(P, W, H, a->num_rendered, 0);  // point_list sits at offset 0
    char* geom = static_cast<char*>(a->geom_buffer);
    char* image = static_cast<char*>(a->image_buffer);
    char* binning = static_cast<char*>(a->binning_buffer);
    if (debug) {
        // what the forward prepared (counters[kCntFwdFlags]; the render backward clears the records
        // bit, so a second backward cannot reuse accumulated records)
        uint32_t ff = 0;
        LSR_TRY(hipMemcpyAsync(&ff, image + L.counters + 4 * kCntFwdFlags, 4, hipMemcpyDeviceToHost, stream),
                "read forward flags");
        LSR_TRY(hipStreamSynchronize(stream), "read forward flags");
        if ((a->flags & LSR_BWD_RECORDS_ZEROED) && !(ff & kFwdZeroedRecords))
            return fail(LSR_ERR_INVALID, "lsr_backward: LSR_BWD_RECORDS_ZEROED, but the forward did not clear the "
                                         "records (LSR_FWD_ZERO_GRAD_RECORDS) or they were used by a backward");
        if (a->dL_dloss && !(ff & kFwdFusedLoss))
            return fail(LSR_ERR_INVALID, "lsr_backward: dL_dloss, but the forward did not fuse the loss");
        if (a->dL_dout_color && (ff & kFwdNoColorState))
            return fail(LSR_ERR_INVALID, "lsr_backward: dL_dout_color, but the forward was told no colour gradient "
                                         "follows (LSR_FWD_NO_COLOR_GRAD)");
        if (ff & kFwdNoBackward)
            return fail(LSR_ERR_INVALID, "lsr_backward: the forward was told no backward follows (LSR_FWD_NO_BACKWARD)");
    }
    // the render backward's 5-value form (no geometry, no colour gradient) keeps 20-B records; the
    // first backward of a forward that cleared them (LSR_FWD_ZERO_GRAD_RECORDS) uses them directly
    const bool compact = !geometry && !a->dL_dout_color;
    const int stride = compact ? kGradStrideLang : kGradStride;
    float* grad = nullptr;
    if (compact && (a->flags & LSR_BWD_RECORDS_ZEROED)) {
        grad = reinterpret_cast<float*>(geom + L.grad_records);
    } else if (defer) {  // (update implies the compact form) the records stay for lsr_language_tail
        grad = reinterpret_cast<float*>(geom + L.grad_records);
        LSR_TRY(zero_fill(grad, 4 * ((size_t)kGradStrideLang * (size_t)P + kDeferXyOffset), stream),
                "memset grad records");
    } else {
        grad = static_cast<float*>(alloc(user, LSR_BUF_BACKWARD, lsr_backward_bytes(P)));
        if (!grad) return fail(LSR_ERR_ALLOC, "lsr_backward: gradient scratch allocation failed");
        LSR_TRY(zero_fill(grad, 4 * (size_t)stride * (size_t)P, stream), "memset grad");
    }

    RenderParams rp = walk_params(W, H, L, geom, image, binning);
    rp.include_feature = (s->include_feature && a->language_feature) ? 1 : 0;
    if (a->flags & LSR_BIND_BACKWARD) rp.bind = reinterpret_cast<const ViewBind*>(geom + L.view_bind);
    rp.bg = s->bg;
    rp.dL_dcolor = a->dL_dout_color;
    rp.dL_dlang = a->dL_dout_language_feature;
    rp.dL_dloss = a->dL_dloss;
    rp.loss_code = reinterpret_cast<uint8_t*>(image + L.loss_code);
    rp.grad = grad;
    if (defer) {  // planar records (LSR_BWD_DEFER_TAIL), the skip flag after the language partials
        rp.grad_xy = grad + 3 * (size_t)P + kDeferXyOffset;
        rp.flag_src = a->update_skip;
        rp.flag_dst = reinterpret_cast<int32_t*>(grad + 3 * (size_t)P);
    }
    rp.fwd_flags = reinterpret_cast<uint32_t*>(image + L.counters) + kCntFwdFlags;
    rp.geo = geometry ? 1 : 0;
    rp.shared_cu = (a->flags & LSR_BWD_SHARED_CU) ? 1 : 0;
    if (a->num_rendered > 0) {
        LSR_TRY(launch_render_backward(rp, L.tiles, stream), "render backward");
    } else if (defer) {  // no render backward: the flag word by a copy
        if (a->update_skip)
            LSR_TRY(hipMemcpyAsync(rp.flag_dst, a->update_skip, 4, hipMemcpyDeviceToDevice, stream), "copy skip flag");
        else
            LSR_TRY(zero_fill(rp.flag_dst, 4, stream), "clear skip flag");
    }
    if (a->update) {
        if (defer) return LSR_OK;  // lsr_language_tail runs the rest after the caller's all-reduce
        // the language step's tail in one pass: epilogue + Adam (+ the next forward's feature slots)
        const lsr_adam_tensor& u = *a->update;
        LSR_TRY(launch_language_tail(P, a->radii, grad, const_cast<float*>(a->language_feature), u.exp_avg, u.exp_avg_sq,
                                     a->dL_dmeans2D, a->dL_dlanguage_feature, adam_hyper(u), a->update_step_dev,
                                     a->update_skip,
                                     reinterpret_cast<float4*>(a->fill_record), 0, stream,
                                     (a->flags & LSR_BIND_FILL_PLANE) ? 1 : 0),
                "language tail");
        return LSR_OK;
    }
    if (!geometry) {
        LSR_TRY(launch_grad_epilogue(P, a->radii, grad, stride, a->language_feature,
                                     (a->raw & LSR_RAW_LANGUAGE) ? 1 : 0, a->dL_dmeans2D,
                                     rp.include_feature ? a->dL_dlanguage_feature : nullptr, stream),
                "gradient epilogue");
        if (!rp.include_feature && a->dL_dlanguage_feature)
            LSR_TRY(zero_fill(a->dL_dlanguage_feature, (size_t)P * 3 * 4, stream), "memset dlang");
        return LSR_OK;
    }

    PreprocessBwdParams bp{};
    bp.P = P;
    bp.M = a->M;
    bp.D = s->sh_degree;
    bp.W = W;
    bp.H = H;
    bp.tanfovx = s->tanfovx;
    bp.tanfovy = s->tanfovy;
    bp.focal_y = (float)H / (2.0f * s->tanfovy);
    bp.focal_x = (float)W / (2.0f * s->tanfovx);
    bp.scale_modifier = s->scale_modifier;
    bp.means = a->means3D;
    bp.shs = a->shs;
    bp.scales = a->scales;
    bp.rots = a->rotations;
    bp.cov_pre = a->cov3D_precomp;
    bp.view = s->viewmatrix;
    bp.proj = s->projmatrix;
    bp.campos = s->campos;
    bp.radii = a->radii;
    bp.clamped = reinterpret_cast<const uint32_t*>(geom + L.clamped);
    bp.grad = grad;
    bp.dmeans2D = a->dL_dmeans2D;
    bp.dcolors = a->dL_dcolors;
    bp.dlang = a->dL_dlanguage_feature;
    bp.dopac = a->dL_dopacity;
    bp.dmeans3D = a->dL_dmeans3D;
    bp.dcov = a->dL_dcov3D;
    bp.dsh = a->shs ? a->dL_dsh : nullptr;
    bp.dscales = a->dL_dscales;
    bp.drots = a->dL_drotations;
    bp.raw = a->raw;
    bp.opac = a->opacities;
    bp.lang = a->language_feature;
    bp.shs_rest = a->shs_rest;
    bp.dsh_rest = a->dL_dsh_rest;
    if (!a->shs && a->dL_dsh && a->M > 0)
        LSR_TRY(zero_fill(a->dL_dsh, (size_t)P * a->M * 3 * 4, stream), "memset dsh");
    LSR_TRY(launch_preprocess_backward(bp, stream), "preprocess backward");
    return LSR_OK;
}

size_t lsr_view_pack_bytes(int32_t P, int32_t width, int32_t height, int64_t num_rendered)
{
    if (P < 1 || width < 1 || height < 1 || num_rendered < 0) return 0;
    return make_view_pack(P, width, height, num_rendered).geometry_bytes;
}

size_t lsr_view_plan_pack_bytes(int32_t P, int32_t width, int32_t height, int64_t num_rendered)
{
    if (P < 1 || width < 1 || height < 1 || num_rendered < 0) return 0;
    return make_view_pack(P, width, height, num_rendered).bytes;
}

int32_t lsr_view_plan_layout(int32_t P, int32_t width, int32_t height, int64_t capacity_rendered, int64_t num_rendered,
                             lsr_view_plan_offsets* out)
{
    if (P < 1 || width < 1 || height < 1 || capacity_rendered < 1 || num_rendered < 0 ||
        num_rendered > capacity_rendered || !out)
        return fail(LSR_ERR_INVALID, "lsr_view_plan_layout: invalid argument");
    const ViewPack V = make_view_pack(P, width, height, num_rendered);
    const Layout L = make_layout(P, width, height, capacity_rendered, 0);
    out->pack_counters = V.counters;
    out->pack_cover = V.cover;
    out->pack_bytes = V.bytes;
    out->set_counters = L.counters;
    out->set_cover = L.cover;
    out->set_final_T = L.final_T;
    out->set_n_contrib = L.n_contrib;
    out->set_split_desc = L.split_desc;
    out->set_bwd_lists = L.tile_lists + 4 * (size_t)kWorkClasses * (size_t)L.tiles;
    out->set_loss_code = L.loss_code;
    out->tiles = (size_t)L.tiles;
    out->classes = kWorkClasses;
    out->split_items = kSplitItems;
    out->word_plan_ready = kCntPlanReady;
    out->word_bwd_class = kCntBwdClass;
    return LSR_OK;
}

int32_t lsr_view_counts(int32_t width, int32_t height, const void* image, uint32_t* host_counters, void* stream_ptr)
{
    if (width < 1 || height < 1 || !image || !host_counters ||
        ((reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(host_counters)) & 3) != 0)
        return fail(LSR_ERR_INVALID, "lsr_view_counts: a positive image size, the image buffer and 8 words of pinned "
                                     "host memory are needed");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    const Layout L = make_layout(0, width, height, 0, 0);
    LSR_TRY(launch_view_counts(reinterpret_cast<const uint32_t*>(static_cast<const char*>(image) + L.counters),
                               host_counters, stream),
            "view counts");
    return LSR_OK;
}

// The checks of a view call's args (a not null) that lsr_view_save / lsr_view_restore and lsr_view_bind
// share, in each one's order; null when they pass.  pack_optional (lsr_view_bind): no pack is a miss, and
// num_rendered and pack_bytes are then not looked at; a null buffer (null_buffer_text) answers before
// num_rendered there, after it in the copies.
static const char* view_args_error(const lsr_view_args* a, bool pack_optional, const char* null_buffer_text)
{
    if (a->P < 1 || a->width < 1 || a->height < 1 || a->width > 65535 * kTile || a->height > 65535 * kTile)
        return "P, width and height must be positive";
    if (a->capacity_rendered < 1 || a->capacity_entries < 1 || a->capacity_rendered > 0xFFFFFFFFll ||
        a->capacity_entries > 0xFFFFFFFFll)
        return "the capacities must be positive (both < 2^32)";
    const bool buffers = a->geom && a->image && a->binning && a->radii && (pack_optional || a->pack);
    if (pack_optional && !buffers) return null_buffer_text;
    if (a->pack || !pack_optional) {
        if (a->num_rendered < 0 || a->num_rendered > a->capacity_rendered)
            return "num_rendered must be 0 .. capacity_rendered";
        if (!buffers) return null_buffer_text;
        if (a->pack_bytes < lsr_view_pack_bytes(a->P, a->width, a->height, a->num_rendered))
            return "pack_bytes is below lsr_view_pack_bytes";
    }
    if (((reinterpret_cast<uintptr_t>(a->geom) | reinterpret_cast<uintptr_t>(a->image) |
          reinterpret_cast<uintptr_t>(a->binning) | reinterpret_cast<uintptr_t>(a->pack)) & 15) != 0 ||
        (reinterpret_cast<uintptr_t>(a->radii) & 3) != 0)
        return "the buffers and the pack must be 16-byte aligned";
    if (a->reserved != 0 || (a->flags & ~(LSR_FWD_ZERO_GRAD_RECORDS | LSR_FWD_NO_COLOR_GRAD | LSR_FWD_NO_BACKWARD)))
        return "unknown flag";
    return nullptr;
}

// ViewParams of a view call; the caller sets R, overflow and plan_room, whose rules differ
static ViewParams view_params(const lsr_view_args* a)
{
    ViewParams v{};
    v.P = a->P;
    v.W = a->width;
    v.H = a->height;
    v.R_cap = a->capacity_rendered;
    v.geom = static_cast<char*>(a->geom);
    v.image = static_cast<char*>(a->image);
    v.binning = static_cast<char*>(a->binning);
    v.pack = static_cast<char*>(a->pack);
    v.radii = a->radii;
    v.fwd_flags = forward_flags_word(a->flags, a->fused_loss != 0);
    return v;
}

static int32_t view_copy(const lsr_view_args* a, void* stream_ptr, bool restore)
{
    const char* who = restore ? "lsr_view_restore" : "lsr_view_save";
    if (!a) return invalid(who, "null argument");
    if (const char* why = view_args_error(a, false, "null buffer")) return invalid(who, why);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    ViewParams v = view_params(a);
    v.R = a->num_rendered;
    v.overflow = restore ? a->overflow : nullptr;
    v.plan_room = a->pack_bytes >= lsr_view_plan_pack_bytes(a->P, a->width, a->height, a->num_rendered);
    LSR_TRY(launch_view_copy(v, restore, stream), restore ? "view restore" : "view save");
    return LSR_OK;
}

int32_t lsr_view_save(const lsr_view_args* a, void* stream) { return view_copy(a, stream, false); }

int32_t lsr_view_bind_layout(int32_t P, int32_t width, int32_t height, size_t* plane, size_t* table)
{
    if (P < 0 || width < 0 || height < 0 || !plane || !table)
        return fail(LSR_ERR_INVALID, "lsr_view_bind_layout: invalid argument");
    const Layout L = make_layout(P, width, height, 0, 0);
    *plane = L.lang_plane;
    *table = L.view_bind;
    return LSR_OK;
}

int32_t lsr_view_bind(const lsr_view_args* a, int32_t bind_flags, void* stream_ptr)
{
    static const char who[] = "lsr_view_bind";
    if (!a) return invalid(who, "null argument");
    if (bind_flags & ~LSR_BIND_CLAMPED) return invalid(who, "unknown bind flag");
    if (const char* why = view_args_error(a, true, "null buffer (the set's table and plane live in its geometry buffer)"))
        return invalid(who, why);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    ViewParams v = view_params(a);
    v.R = a->pack ? a->num_rendered : 0;
    v.overflow = a->pack ? a->overflow : nullptr;
    v.plan_room = a->pack && a->pack_bytes >= lsr_view_plan_pack_bytes(a->P, a->width, a->height, a->num_rendered);
    LSR_TRY(launch_view_bind(v, (bind_flags & LSR_BIND_CLAMPED) != 0, stream), "view bind");
    return LSR_OK;
}

int32_t lsr_view_restore(const lsr_view_args* a, void* stream) { return view_copy(a, stream, true); }

int32_t lsr_profile_enable(int32_t on)
{
    std::lock_guard<std::mutex> g(g_prof.mu);
    g_prof.drain();
    if (on) {
        g_prof.stats.clear();
        // events come from a pool filled here, not created inside the measured launches
        while (g_prof.pool.size() < 512) {
            hipEvent_t e = nullptr;
            if (hipEventCreateWithFlags(&e, kEventFlags) != hipSuccess) break;
            g_prof.pool.push_back(e);
        }
    }
    g_prof.on = on != 0;
    return LSR_OK;
}

int32_t lsr_profile_sample(int32_t every)
{
    if (every < 1) return fail(LSR_ERR_INVALID, "lsr_profile_sample: every must be >= 1");
    std::lock_guard<std::mutex> g(g_prof.mu);
    g_prof.every = every;
    g_prof.seen = 0;
    return LSR_OK;
}

int32_t lsr_profile_select(const char* stages)
{
    std::lock_guard<std::mutex> g(g_prof.mu);
    g_prof.select.clear();
    if (!stages) return LSR_OK;
    std::string cur;
    for (const char* c = stages;; c++) {
        if (*c == ',' || *c == 0) {
            if (!cur.empty()) g_prof.select.push_back(cur);
            cur.clear();
            if (*c == 0) break;
        } else {
            cur.push_back(*c);
        }
    }
    return LSR_OK;
}

int32_t lsr_profile_report(lsr_kernel_stat* out, int32_t capacity)
{
    std::lock_guard<std::mutex> g(g_prof.mu);
    g_prof.drain();
    int32_t n = 0;
    for (auto& kv : g_prof.stats) {
        if (out && n < capacity) {
            memset(out[n].name, 0, sizeof(out[n].name));
            strncpy(out[n].name, kv.first.c_str(), sizeof(out[n].name) - 1);
            out[n].launches = kv.second.first;
            out[n].total_ms = kv.second.second;
        }
        n++;
    }
    return n;
}

int32_t lsr_debug_render_stats(uint64_t* out, int32_t n)
{
    if (!out || n <= 0) return fail(LSR_ERR_INVALID, "lsr_debug_render_stats: invalid argument");
    const bool debug = false;
    hipStream_t stream = nullptr;
    (void)stream;
    LSR_TRY(render_stats_read(reinterpret_cast<unsigned long long*>(out), n), "render stats");
    return LSR_OK;
}

int32_t lsr_debug_render_timeline(int32_t kernel, uint32_t* out, int32_t n)
{
    if (!out || n <= 0 || kernel < 0 || kernel > 1)
        return fail(LSR_ERR_INVALID, "lsr_debug_render_timeline: invalid argument");
    const bool debug = false;
    hipStream_t stream = nullptr;
    (void)stream;
    LSR_TRY(render_timeline_read(out, kernel, n), "render timeline");
    return LSR_OK;
}

int32_t lsr_debug_scan_stalls(void)
{
    hipError_t herr = hipSuccess;
    HostBlock* hb = t_host.get(&herr);
    if (!hb) return -fail(LSR_ERR_HIP, "lsr_debug_scan_stalls: pinned host block", herr);
    return (int32_t)__atomic_exchange_n(&hb->stall, 0u, __ATOMIC_ACQ_REL);
}

uint32_t lsr_debug_set_spin_limit(uint32_t limit) { return set_stall_spin_limit(limit); }

int32_t lsr_debug_bucket_timeline(uint32_t* out, int32_t n)
{
    if (!out || n <= 0) return fail(LSR_ERR_INVALID, "lsr_debug_bucket_timeline: invalid argument");
    const bool debug = false;
    hipStream_t stream = nullptr;
    (void)stream;
    LSR_TRY(bucket_timeline_read(out, n), "bucket timeline");
    return LSR_OK;
}

int32_t lsr_debug_clock_probe(uint64_t* out_device, void* stream_ptr)
{
    if (!out_device) return fail(LSR_ERR_INVALID, "lsr_debug_clock_probe: invalid argument");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    LSR_TRY(launch_clock_probe(out_device, stream), "clock probe");
    return LSR_OK;
}

int32_t lsr_graph_launch(void* graph_exec, void* stream_ptr, void* const* wait_events, int32_t n_waits,
                         void* record_event)
{
    if (!graph_exec || n_waits < 0 || (n_waits > 0 && !wait_events))
        return fail(LSR_ERR_INVALID, "lsr_graph_launch: invalid argument");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    hipError_t e;
    for (int32_t i = 0; i < n_waits; i++)
        if ((e = hipStreamWaitEvent(stream, reinterpret_cast<hipEvent_t>(wait_events[i]), 0)) != hipSuccess)
            return fail(LSR_ERR_HIP, "lsr_graph_launch: stream wait", e);
    if ((e = hipGraphLaunch(reinterpret_cast<hipGraphExec_t>(graph_exec), stream)) != hipSuccess)
        return fail(LSR_ERR_HIP, "lsr_graph_launch: graph launch", e);
    if (record_event && (e = hipEventRecord(reinterpret_cast<hipEvent_t>(record_event), stream)) != hipSuccess)
        return fail(LSR_ERR_HIP, "lsr_graph_launch: event record", e);
    return LSR_OK;
}

int32_t lsr_query_relevancy(const lsr_query_args* a, void* stream_ptr)
{
    if (!a) return fail(LSR_ERR_INVALID, "lsr_query_relevancy: null args");
    if (a->N < 0 || a->N > (int64_t)INT32_MAX * kQPix) return fail(LSR_ERR_INVALID, "lsr_query_relevancy: invalid N");
    if (a->n_layers < 1 || a->n_layers > kQueryMaxLayers)
        return fail(LSR_ERR_INVALID, "lsr_query_relevancy: invalid n_layers (1 to 8 layers)");
    if (!a->widths) return fail(LSR_ERR_INVALID, "lsr_query_relevancy: null widths");
    QueryParams p{};
    int off = 0;
    for (int l = 0; l < a->n_layers; l++) {
        const int wd = a->widths[l];
        if (wd < 16 || wd > 512 || wd % 16 != 0)
            return fail(LSR_ERR_INVALID, "lsr_query_relevancy: invalid width (a multiple of 16, at most 512)");
        p.widths[l] = wd;
        p.w_off[l] = off;
        off += wd * (l ? a->widths[l - 1] : 3) + wd;
    }
    if (a->n_pos < 1 || a->n_neg < 1 || a->n_pos + a->n_neg > 64)
        return fail(LSR_ERR_INVALID, "lsr_query_relevancy: invalid phrase counts (n_pos >= 1, n_neg >= 1, at most 64)");
    if (!a->feature || !a->weights || !a->phrases || !a->out_relevancy)
        return fail(LSR_ERR_INVALID, "lsr_query_relevancy: null pointer");
    if (((reinterpret_cast<uintptr_t>(a->weights) | reinterpret_cast<uintptr_t>(a->phrases)) & 15) != 0)
        return fail(LSR_ERR_INVALID, "lsr_query_relevancy: weights and phrases must be 16-byte aligned");
    p.N = a->N;
    p.feature = a->feature;
    p.channel_stride = a->channel_stride;
    p.pixel_stride = a->pixel_stride;
    p.n_layers = a->n_layers;
    p.weights = a->weights;
    p.n_pos = a->n_pos;
    p.n_neg = a->n_neg;
    p.phrases = a->phrases;
    p.out_relevancy = a->out_relevancy;
    p.out_decoded = a->out_decoded;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;  // read by LSR_TRY (its sync-and-check after the launch): this call has no debug setting
    LSR_TRY(launch_query(p, stream), "query relevancy");
    return LSR_OK;
}

int32_t lsr_query_semantic(const lsr_query_semantic_args* a, void* stream_ptr)
{
    if (!a) return fail(LSR_ERR_INVALID, "lsr_query_semantic: null args");
    if (a->N < 0 || a->N > (int64_t)INT32_MAX * kQPix) return fail(LSR_ERR_INVALID, "lsr_query_semantic: invalid N");
    if (a->n_layers < 1 || a->n_layers > kQueryMaxLayers)
        return fail(LSR_ERR_INVALID, "lsr_query_semantic: invalid n_layers (1 to 8 layers)");
    if (!a->widths) return fail(LSR_ERR_INVALID, "lsr_query_semantic: null widths");
    QueryParams p{};
    int off = 0;
    for (int l = 0; l < a->n_layers; l++) {
        const int wd = a->widths[l];
        if (wd < 16 || wd > 512 || wd % 16 != 0)
            return fail(LSR_ERR_INVALID, "lsr_query_semantic: invalid width (a multiple of 16, at most 512)");
        p.widths[l] = wd;
        p.w_off[l] = off;
        off += wd * (l ? a->widths[l - 1] : 3) + wd;
    }
    if (a->n_labels < 1 || a->n_neg < 1 || a->n_labels + a->n_neg > 64)
        return fail(LSR_ERR_INVALID, "lsr_query_semantic: invalid phrase counts (n_labels >= 1, n_neg >= 1, at most 64)");
    if (!a->feature || !a->weights || !a->phrases || !a->out_label)
        return fail(LSR_ERR_INVALID, "lsr_query_semantic: null pointer");
    if (((reinterpret_cast<uintptr_t>(a->weights) | reinterpret_cast<uintptr_t>(a->phrases)) & 15) != 0)
        return fail(LSR_ERR_INVALID, "lsr_query_semantic: weights and phrases must be 16-byte aligned");
    p.N = a->N;
    p.feature = a->feature;
    p.channel_stride = a->channel_stride;
    p.pixel_stride = a->pixel_stride;
    p.n_layers = a->n_layers;
    p.weights = a->weights;
    p.n_pos = a->n_labels;
    p.n_neg = a->n_neg;
    p.phrases = a->phrases;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    LSR_TRY(launch_query(p, stream, a->out_label, a->out_score), "query semantic");
    return LSR_OK;
}

int32_t lsr_label_stats(const lsr_label_stats_args* a, void* stream_ptr)
{
    if (!a) return fail(LSR_ERR_INVALID, "lsr_label_stats: null args");
    if (a->N < 0 || a->N > kLabelStatsMaxN || a->n_maps < 0) return fail(LSR_ERR_INVALID, "lsr_label_stats: invalid size");
    if (a->n_classes < 1 || a->n_classes > 64) return fail(LSR_ERR_INVALID, "lsr_label_stats: invalid n_classes (1 to 64)");
    if (a->gt_maps != 1 && a->gt_maps != a->n_maps)
        return fail(LSR_ERR_INVALID, "lsr_label_stats: invalid gt_maps (1, or n_maps)");
    if (!a->pred || !a->gt || !a->out_counts || !a->out_totals) return fail(LSR_ERR_INVALID, "lsr_label_stats: null pointer");
    if (((reinterpret_cast<uintptr_t>(a->out_counts) | reinterpret_cast<uintptr_t>(a->out_totals)) & 7) != 0)
        return fail(LSR_ERR_INVALID, "lsr_label_stats: out_counts and out_totals must be 8-byte aligned");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    LSR_TRY(launch_label_stats(*a, stream), "label stats");
    return LSR_OK;
}

// the checks lsr_eval_filter and lsr_eval_masks share; null when the shape is valid
static const char* eval_shape_error(int32_t n_maps, int32_t H, int32_t W)
{
    if (n_maps < 0) return "invalid n_maps";
    if (H < 2 || W < 2) return "invalid size (H and W are at least 2)";
    if ((int64_t)H * (int64_t)W >= ((int64_t)1 << 31)) return "invalid size (H * W must be below 2^31)";
    return nullptr;
}

int32_t lsr_eval_filter(const lsr_eval_filter_args* a, void* stream_ptr)
{
    if (!a) return fail(LSR_ERR_INVALID, "lsr_eval_filter: null args");
    if (const char* why = eval_shape_error(a->n_maps, a->H, a->W)) return invalid("lsr_eval_filter", why);
    if (!a->maps || !a->out_stats) return fail(LSR_ERR_INVALID, "lsr_eval_filter: null pointer");
    if ((reinterpret_cast<uintptr_t>(a->out_stats) & 7) != 0)
        return fail(LSR_ERR_INVALID, "lsr_eval_filter: out_stats must be 8-byte aligned");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    LSR_TRY(launch_eval_filter(*a, stream), "eval filter");
    return LSR_OK;
}

int32_t lsr_eval_masks(const lsr_eval_mask_args* a, void* stream_ptr)
{
    if (!a) return fail(LSR_ERR_INVALID, "lsr_eval_masks: null args");
    if (const char* why = eval_shape_error(a->n_maps, a->H, a->W)) return invalid("lsr_eval_masks", why);
    if (!a->blend || !a->stats || !a->out_mask || (a->gt_mask && !a->out_counts))
        return fail(LSR_ERR_INVALID, "lsr_eval_masks: null pointer");
    if (a->gt_mask && (a->n_prompts < 1 || a->n_maps % a->n_prompts != 0))
        return fail(LSR_ERR_INVALID, "lsr_eval_masks: invalid n_prompts (at least 1, and a divisor of n_maps)");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    LSR_TRY(launch_eval_masks(*a, stream), "eval masks");
    return LSR_OK;
}

int32_t lsr_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                         uint8_t* visible, void* stream_ptr)
{
    if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !projmatrix || !visible)))
        return fail(LSR_ERR_INVALID, "lsr_mark_visible: invalid argument");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    LSR_TRY(launch_mark_visible(P, means3D, viewmatrix, projmatrix, visible, stream), "mark visible");
    return LSR_OK;
}

static int32_t fill_language(int32_t P, const float* language_feature, int32_t raw, const int32_t* radii, float* record,
                             void* stream_ptr, int plane)
{
    if (P < 0 || (P > 0 && (!language_feature || !radii || !record)) ||
        (reinterpret_cast<uintptr_t>(record) & 15) != 0)
        return fail(LSR_ERR_INVALID, plane ? "lsr_fill_language_plane: invalid argument" : "lsr_fill_language: invalid argument");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    LSR_TRY(launch_fill_language(P, language_feature, raw, radii, reinterpret_cast<float4*>(record), stream, plane),
            "fill language");
    return LSR_OK;
}

int32_t lsr_fill_language(int32_t P, const float* language_feature, int32_t raw, const int32_t* radii, float* record,
                          void* stream)
{
    return fill_language(P, language_feature, raw, radii, record, stream, 0);
}

int32_t lsr_fill_language_plane(int32_t P, const float* language_feature, int32_t raw, const int32_t* radii, float* plane,
                                void* stream)
{
    return fill_language(P, language_feature, raw, radii, plane, stream, 1);
}

// planes / H / W >= 1 and a grid that fits: nullptr, or what is wrong
static const char* rgb_loss_shape_error(int32_t planes, int32_t H, int32_t W)
{
    if (planes < 1 || H < 1 || W < 1) return "invalid size (planes, H and W are at least 1)";
    if (rgb_loss_blocks(planes, H, W) > (int64_t)INT32_MAX) return "invalid size (more than 2^31 - 1 tiles)";
    return nullptr;
}

size_t lsr_rgb_loss_scratch_bytes(int32_t planes, int32_t H, int32_t W)
{
    if (planes < 1 || H < 1 || W < 1) return 0;
    return rgb_loss_scratch_bytes(planes, H, W);
}

int32_t lsr_rgb_loss_forward(const lsr_rgb_loss_args* a, void* stream_ptr)
{
    if (!a) return fail(LSR_ERR_INVALID, "lsr_rgb_loss_forward: null args");
    if (const char* why = rgb_loss_shape_error(a->planes, a->H, a->W)) return invalid("lsr_rgb_loss_forward", why);
    if (!a->image || !a->target || !a->out_terms || !a->scratch)
        return fail(LSR_ERR_INVALID, "lsr_rgb_loss_forward: null pointer");
    if ((reinterpret_cast<uintptr_t>(a->scratch) & 7) != 0)
        return fail(LSR_ERR_INVALID, "lsr_rgb_loss_forward: scratch must be 8-byte aligned");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    LSR_TRY(launch_rgb_loss_forward(*a, stream), "rgb loss");
    return LSR_OK;
}

int32_t lsr_rgb_loss_backward(const lsr_rgb_loss_bwd_args* a, void* stream_ptr)
{
    if (!a) return fail(LSR_ERR_INVALID, "lsr_rgb_loss_backward: null args");
    if (const char* why = rgb_loss_shape_error(a->planes, a->H, a->W)) return invalid("lsr_rgb_loss_backward", why);
    if (!a->image || !a->target || !a->maps || !a->dL_dloss || !a->out_dL_dimage)
        return fail(LSR_ERR_INVALID, "lsr_rgb_loss_backward: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    LSR_TRY(launch_rgb_loss_backward(*a, stream), "rgb loss backward");
    return LSR_OK;
}

size_t lsr_masked_l1_scratch_bytes(int32_t C, int64_t HW)
{
    (void)C;
    (void)HW;
    return masked_l1_scratch_bytes();
}

int32_t lsr_masked_l1_forward(int32_t C, int64_t HW, const float* pred, const float* gt, const void* mask,
                              int32_t mask_is_float, float* loss, void* scratch, void* stream_ptr)
{
    if (C <= 0 || HW <= 0 || !pred || !gt || !mask || !loss || !scratch)
        return fail(LSR_ERR_INVALID, "lsr_masked_l1_forward: invalid argument");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    hipError_t herr = hipSuccess;
    HostBlock* hb = t_host.get(&herr);
    if (!hb) return fail(LSR_ERR_HIP, "lsr_masked_l1_forward: pinned host block", herr);
    // per-scratch launch epoch (never 0, the value of freshly zeroed scratch)
    uint32_t epoch = 0;
    {
        static std::mutex mu;
        static std::map<void*, uint32_t> epochs;
        std::lock_guard<std::mutex> g(mu);
        uint32_t& e = epochs[scratch];
        e = e + 1 == 0 ? 1 : e + 1;
        epoch = e;
    }
    LSR_TRY(launch_masked_l1_forward(C, HW, pred, gt, mask, mask_is_float, loss, scratch, epoch, &hb->stall, stream),
            "masked l1");
    return LSR_OK;
}

int32_t lsr_masked_l1_backward(int32_t C, int64_t HW, const float* pred, const float* gt, const void* mask,
                               int32_t mask_is_float, const float* grad_loss, float* grad_pred, void* stream_ptr)
{
    if (C <= 0 || HW <= 0 || !pred || !gt || !mask || !grad_loss || !grad_pred)
        return fail(LSR_ERR_INVALID, "lsr_masked_l1_backward: invalid argument");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    LSR_TRY(launch_masked_l1_backward(C, HW, pred, gt, mask, mask_is_float, grad_loss, grad_pred, stream),
            "masked l1 backward");
    return LSR_OK;
}

int32_t lsr_adam_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, double lr,
                      double beta1, double beta2, double eps, int64_t step, void* stream_ptr)
{
    if (n < 0 || (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq)) || step < 1)
        return fail(LSR_ERR_INVALID, "lsr_adam_step: invalid argument");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    const AdamScalars a = adam_scalars(lr, beta1, beta2, eps, step);
    LSR_TRY(launch_adam(n, param, grad, exp_avg, exp_avg_sq, a, stream), "adam");
    return LSR_OK;
}

int32_t lsr_adam_multi(int32_t count, const lsr_adam_tensor* tensors, float grad_scale, int64_t* step_dev,
                       const int32_t* skip, void* stream_ptr)
{
    if (count < 0 || (count > 0 && !tensors)) return fail(LSR_ERR_INVALID, "lsr_adam_multi: invalid argument");
    if (step_dev && count > kAdamMaxTensors)
        return fail(LSR_ERR_INVALID, "lsr_adam_multi: step_dev allows at most 16 tensors");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    for (int32_t k0 = 0; k0 < count; k0 += kAdamMaxTensors) {
        AdamTable tab{};
        for (int32_t k = k0; k < count && k < k0 + kAdamMaxTensors; k++) {
            const lsr_adam_tensor& t = tensors[k];
            if (t.n < 0 || (t.n > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq)) ||
                (t.step < 1 && !step_dev) || (step_dev && (t.step < -((int64_t)1 << 40) || t.step > ((int64_t)1 << 40))))
                return fail(LSR_ERR_INVALID, "lsr_adam_multi: invalid tensor entry");
            if (t.n == 0) continue;
            tab.hyper[tab.count] = AdamHyper{t.lr, t.beta1, t.beta2, t.eps, step_dev ? t.step : 0};
            AdamSegment& g = tab.seg[tab.count++];
            g.param = t.param;
            g.grad = t.grad;
            g.m = t.exp_avg;
            g.v = t.exp_avg_sq;
            g.n = t.n;
            g.a = adam_scalars(t.lr, t.beta1, t.beta2, t.eps, t.step < 1 ? 1 : t.step);
        }
        tab.step_dev = step_dev;
        tab.skip = skip;
        LSR_TRY(launch_adam_multi(tab, grad_scale, stream), "adam");
    }
    return LSR_OK;
}

static int32_t adam_fill_language(const lsr_adam_tensor* t, float grad_scale, int64_t* step_dev, const int32_t* skip,
                                  void* fill_record, int32_t raw, void* stream_ptr, int plane)
{
    if (!t || !step_dev || !fill_record || t->n < 0 || t->n % 3 != 0 || t->n / 3 > INT32_MAX ||
        (t->n > 0 && (!t->param || !t->grad || !t->exp_avg || !t->exp_avg_sq)) ||
        t->step < -((int64_t)1 << 40) || t->step > ((int64_t)1 << 40))
        return fail(LSR_ERR_INVALID, "lsr_adam_fill_language: invalid argument");
    if (reinterpret_cast<uintptr_t>(fill_record) & 15)
        return fail(LSR_ERR_INVALID, "lsr_adam_fill_language: fill_record must be 16-byte aligned");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    LSR_TRY(launch_adam_fill((int)(t->n / 3), t->grad, grad_scale, t->param, t->exp_avg, t->exp_avg_sq, adam_hyper(*t),
                             step_dev, skip, reinterpret_cast<float4*>(fill_record), raw, stream, plane),
            "adam fill");
    return LSR_OK;
}

int32_t lsr_adam_fill_language(const lsr_adam_tensor* t, float grad_scale, int64_t* step_dev, const int32_t* skip,
                               void* fill_record, int32_t raw, void* stream)
{
    return adam_fill_language(t, grad_scale, step_dev, skip, fill_record, raw, stream, 0);
}

int32_t lsr_adam_fill_language_plane(const lsr_adam_tensor* t, float grad_scale, int64_t* step_dev, const int32_t* skip,
                                     void* fill_plane, int32_t raw, void* stream)
{
    return adam_fill_language(t, grad_scale, step_dev, skip, fill_plane, raw, stream, 1);
}

int32_t lsr_language_tail(const lsr_settings* s, const lsr_backward_args* a, void* stream_ptr)
{
    if (!s || !a) return fail(LSR_ERR_INVALID, "lsr_language_tail: null argument");
    const int P = a->P, W = s->image_width, H = s->image_height;
    if (P < 0 || W <= 0 || H <= 0) return fail(LSR_ERR_INVALID, "lsr_language_tail: invalid P or image size");
    if (!a->update || !a->update_step_dev || !a->dL_dlanguage_feature || !(a->raw & LSR_RAW_LANGUAGE) ||
        !a->language_feature || a->update->param != a->language_feature || a->update->n != 3 * (int64_t)P ||
        !a->update->exp_avg || !a->update->exp_avg_sq)
        return fail(LSR_ERR_INVALID, "lsr_language_tail: the arguments of a fused update (lsr_backward_args.update) "
                                     "are needed");
    if (P > 0 && (!a->geom_buffer || !a->radii)) return fail(LSR_ERR_INVALID, "lsr_language_tail: missing forward state");
    if (a->fill_record && (reinterpret_cast<uintptr_t>(a->fill_record) & 15))
        return fail(LSR_ERR_INVALID, "lsr_language_tail: fill_record must be 16-byte aligned");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = s->debug != 0;
    const Layout L = make_layout(P, W, H, a->num_rendered, 0);
    float* grad = P > 0 ? reinterpret_cast<float*>(static_cast<char*>(a->geom_buffer) + L.grad_records) : nullptr;
    const lsr_adam_tensor& u = *a->update;
    // the skip flag the all-reduce carried (the word after the language partials): any rank's overflow
    const int32_t* skip = P > 0 ? reinterpret_cast<const int32_t*>(grad + 3 * (size_t)P) : a->update_skip;
    LSR_TRY(launch_language_tail(P, a->radii, grad, const_cast<float*>(a->language_feature), u.exp_avg, u.exp_avg_sq,
                                 a->dL_dmeans2D, a->dL_dlanguage_feature, adam_hyper(u), a->update_step_dev, skip,
                                 reinterpret_cast<float4*>(a->fill_record), 1, stream,
                                 (a->flags & LSR_BIND_FILL_PLANE) ? 1 : 0),
            "language tail");
    return LSR_OK;
}

int32_t lsr_densification_stats(int32_t P, const int32_t* radii, const float* dL_dmeans2D, float* max_radii2D,
                                float* xyz_gradient_accum, float* denom, void* stream_ptr)
{
    if (P < 0 || (P > 0 && (!radii || !dL_dmeans2D)))
        return fail(LSR_ERR_INVALID, "lsr_densification_stats: invalid argument");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    LSR_TRY(launch_densification_stats(P, radii, dL_dmeans2D, max_radii2D, xyz_gradient_accum, denom, stream),
            "densification stats");
    return LSR_OK;
}

int32_t lsr_dist_cuda2(int64_t N, const float* points, float* out_mean_dist, lsr_alloc_fn alloc, void* user,
                       void* stream_ptr)
{
    if (N < 0 || (N > 0 && (!points || !out_mean_dist || !alloc)) || N > 0x3FFFFFFF)
        return fail(LSR_ERR_INVALID, "lsr_dist_cuda2: invalid argument");
    if (N == 0) return LSR_OK;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    void* scratch = alloc(user, LSR_BUF_BACKWARD, knn_scratch_bytes(N));
    if (!scratch) return fail(LSR_ERR_ALLOC, "lsr_dist_cuda2: scratch allocation failed");
    hipError_t herr = hipSuccess;
    HostBlock* hb = t_host.get(&herr);
    if (!hb) return fail(LSR_ERR_HIP, "lsr_dist_cuda2: pinned host block", herr);
    LSR_TRY(launch_knn_mean_dist3(N, points, out_mean_dist, scratch, &hb->stall, stream), "dist_cuda2");
    return LSR_OK;
}

int32_t lsr_debug_knn_grid(const float* box, int64_t N, float* out_origin_h, int32_t* out_dims)
{
    if (!box || !out_origin_h || !out_dims || N < 1 || N > 0x3FFFFFFF)
        return fail(LSR_ERR_INVALID, "lsr_debug_knn_grid: invalid argument");
    knn_debug_grid(box, N, out_origin_h, out_dims);
    return LSR_OK;
}

int32_t lsr_decode_language_feature(int32_t L, int32_t H, int32_t W, const int64_t* seg_map, int32_t level,
                                    int32_t N, int32_t D, const float* feature_map, float* out_feature,
                                    uint8_t* out_mask, void* stream_ptr)
{
    if (L <= 0 || H <= 0 || W <= 0 || level < 0 || level >= L || N <= 0 || D <= 0 || !seg_map || !feature_map ||
        !out_feature || !out_mask)
        return fail(LSR_ERR_INVALID, "lsr_decode_language_feature: invalid argument");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_ptr);
    const bool debug = false;
    hipError_t herr = hipSuccess;
    HostBlock* hb = t_host.get(&herr);
    if (!hb) return fail(LSR_ERR_HIP, "lsr_decode_language_feature: pinned host block", herr);
    __atomic_store_n(&hb->bad_segment, 0u, __ATOMIC_RELEASE);
    LSR_TRY(launch_decode_language_feature(H, W, seg_map + (int64_t)level * H * W, N, D, feature_map, out_feature,
                                           out_mask, &hb->bad_segment, stream),
            "decode language feature");
    // once per view: wait, so that an id the reference's feature_map[seg] would reject is reported
    LSR_TRY(hipStreamSynchronize(stream), "decode language feature (sync)");
    if (__atomic_exchange_n(&hb->bad_segment, 0u, __ATOMIC_ACQ_REL))
        return fail(LSR_ERR_INVALID, "lsr_decode_language_feature: segment id outside [-N, N) of the feature map");
    return LSR_OK;
}

}  // extern "C"
