// lsr_viewcache.hip -- lsr_view_save / lsr_view_restore: a view's frozen geometry as one compact pack.
//
// In LangSplat's language stage every geometry parameter is frozen (scene/gaussian_model.py:203-217),
// so what LSR_PHASE_GEOMETRY (preprocess, depth order, binning) leaves for a given camera is the same
// at every step.  k_view_copy<false> gathers the part of it the later phases read -- the composite
// phase, lsr_backward (language step and all-gradients step) and lsr_language_tail -- into a pack;
// k_view_copy<true> scatters a pack back into a buffer set of the same capacities and re-initialises
// the words the geometry phase clears on every run.  One launch each, grid-stride over the segments,
// consecutive lanes on consecutive 16-byte words; no LDS.
//
// What is kept (make_view_pack), read off render_forward_and_finish, lsr_backward's parameter setup and
// make_layout:
//   counters   the published slots (tile instances, error, super-tile entries, key range) and the
//              forward's class counts of the longest-first schedule (k_bin_emit's)
//   rec01      record[3 i], record[3 i + 1]: position, conic, opacity, r, g
//   recb       word 0 of record[3 i + 2]: b.  Its other three words are the language slots, which
//              belong to the feature fill (a fused update may write them before, while or after a
//              restore runs, as with the geometry call): never read, never written here
//   radii, clamped (the all-gradients backward's preprocess backward reads clamped)
//   ranges     the tiles' [start, end) in the point list
//   order      the forward's class lists, compacted: the scheduled tiles class by class, ascending
//              class, each class in its list's order (workgroup b's tile, and with it the order in
//              which the fused loss adds the workgroups' shares, is what it was)
//   point_list the num_rendered entries
// and the walk plan, which a view's first compositing derives from that geometry alone and which is
// still in the set when the set is next visited (nothing between the render forward and that visit
// rewrites it: the backward only reads it):
//   cover      the R instances' cover masks (entry_cover)
// valid when the saved counters' kCntPlanReady is set (the render forward sets it, the geometry phase
// clears it): a pack saved before any compositing has no plan, and binds as the plain bound form.
// Not kept: depth keys, sort and scan scratch, super-tile tables (geometry-internal); split states,
// the backward's class counts and lists, final_T, n_contrib, loss codes (the compositing writes them
// at every step); the language slots; the gradient records (cleared by the compositing or the backward).
#include "lsr_internal.h"

namespace lsr {

namespace {

constexpr int kViewThreads = 256;
// the guides' cap for memory-bound grids on this chip (256 CUs x 8 blocks), grid-stride beyond
constexpr int kViewMaxBlocks = 2048;

// (kSegCover, the walk plan: save only, into a pack with room for it)
enum ViewSeg : int { kSegRecord, kSegPointList, kSegRadii, kSegClamped, kSegRanges, kSegOrder, kSegCounters, kSegLoss, kSegCover, kSegs };

struct ViewCopy {
    size_t end[kSegs];  // running ends of the segments' item ranges
    int P, T;
    int64_t R;
    int radii_vec;      // radii is 16-byte aligned
    uint32_t fwd_flags; // restore: counters[kCntFwdFlags]
    float4* record;
    int32_t* radii;
    uint4* clamped;
    uint4* ranges;
    uint32_t* lists;
    uint4* point_list;
    uint32_t* counters;
    uint4* loss_words;
    int32_t* overflow;
    uint32_t* pk_counters;
    float4* pk_rec01;
    float* pk_recb;
    int32_t* pk_radii;
    uint4* pk_clamped;
    uint4* pk_ranges;
    uint32_t* pk_order;
    uint4* pk_point_list;
    // the walk plan
    uint4 *cover, *pk_cover;
    int plan_room;  // the pack has the plan's segment (else it ends after the point list)
};

template <bool kRestore, typename T>
__device__ __forceinline__ void move(T* set, T* pack, size_t i)
{
    if (kRestore)
        set[i] = pack[i];
    else
        pack[i] = set[i];
}

// radii item q: Gaussians 4 q .. 4 q + 3
template <bool kRestore>
__device__ __forceinline__ void move_radii(const ViewCopy& p, size_t q)
{
    if (p.radii_vec && 4 * q + 4 <= (size_t)p.P) {
        move<kRestore>(reinterpret_cast<int4*>(p.radii), reinterpret_cast<int4*>(p.pk_radii), q);
    } else {  // the caller's array ends at P and may sit at any 4-byte address
        for (size_t j = 4 * q; j < 4 * q + 4 && j < (size_t)p.P; j++) move<kRestore>(p.radii, p.pk_radii, j);
    }
}

// scheduled slot j: its class from the class counts (the pack's when restoring: the set's are written
// by the same launch), then the list element
template <bool kRestore>
__device__ __forceinline__ void move_order(const ViewCopy& p, uint32_t j)
{
    const uint32_t* cnt = (kRestore ? p.pk_counters : p.counters) + kCntFwdClass;
    uint32_t first = 0;
    for (int c = 0; c < kWorkClasses; c++) {
        const uint32_t n = min(cnt[c], (uint32_t)p.T);
        if (j - first < n) {
            uint32_t* slot = p.lists + (size_t)c * p.T + (j - first);
            if (kRestore)
                *slot = p.pk_order[j];
            else
                p.pk_order[j] = *slot;
            break;
        }
        first += n;  // (j >= first still holds)
    }
}

// counter word c of a set that receives a pack, as k_publish_counters leaves it: the five published
// values, the forward's flags, the forward's class counts; every other word 0 (the overflow word, the
// backward's class counts that the compositing adds to)
__device__ __forceinline__ void restore_counter(const ViewCopy& p, int c)
{
    uint32_t v = 0u;
    if (c == kCntRendered || c == kCntError || c == kCntSuper || c == kCntKeyMin || c == kCntKeyMax ||
        (c >= kCntFwdClass && c < kCntBwdClass))
        v = p.pk_counters[c];
    else if (c == kCntFwdFlags)
        v = p.fwd_flags;
    p.counters[c] = v;
    if (c == kCntOverflow && p.overflow) *p.overflow = 0;
}

template <bool kRestore>
__global__ __launch_bounds__(kViewThreads) void k_view_copy(ViewCopy p)
{
    const size_t stride = (size_t)gridDim.x * kViewThreads;
    for (size_t i = (size_t)blockIdx.x * kViewThreads + threadIdx.x; i < p.end[kSegs - 1]; i += stride) {
        if (i < p.end[kSegRecord]) {
            // float4 k of the record array: Gaussian g = k / 3, word w = k % 3
            const size_t g = i / 3;
            const int w = (int)(i - 3 * g);
            if (w < 2) {
                if (kRestore)
                    p.record[i] = p.pk_rec01[i - g];
                else
                    p.pk_rec01[i - g] = p.record[i];
            } else {  // b only: the language slots stay as they are
                float* b = reinterpret_cast<float*>(p.record + i);
                if (kRestore)
                    *b = p.pk_recb[g];
                else
                    p.pk_recb[g] = *b;
            }
        } else if (i < p.end[kSegPointList]) {
            // (both arrays are padded past 4 ceil(R / 4) entries)
            move<kRestore>(p.point_list, p.pk_point_list, i - p.end[kSegRecord]);
        } else if (i < p.end[kSegRadii]) {
            move_radii<kRestore>(p, i - p.end[kSegPointList]);
        } else if (i < p.end[kSegClamped]) {
            move<kRestore>(p.clamped, p.pk_clamped, i - p.end[kSegRadii]);
        } else if (i < p.end[kSegRanges]) {
            move<kRestore>(p.ranges, p.pk_ranges, i - p.end[kSegClamped]);
        } else if (i < p.end[kSegOrder]) {
            move_order<kRestore>(p, (uint32_t)(i - p.end[kSegRanges]));
        } else if (i < p.end[kSegCounters]) {
            const int c = (int)(i - p.end[kSegOrder]);
            if (!kRestore)  // (a pack without room for the plan says it has none)
                p.pk_counters[c] = c == kCntPlanReady && !p.plan_room ? 0u : p.counters[c];
            else
                restore_counter(p, c);
        } else if (i < p.end[kSegLoss]) {  // restore: the fused loss's words start at 0 (the preprocess clears them)
            p.loss_words[i - p.end[kSegCounters]] = make_uint4(0u, 0u, 0u, 0u);
        } else {  // (save only)
            move<kRestore>(p.cover, p.pk_cover, i - p.end[kSegLoss]);
        }
    }
}

// lsr_view_bind.  Segment kSegRecord is the plane's b word (one Gaussian per item), kSegPointList the
// table (one item); the other segments are k_view_copy<true>'s.  identity (no pack): the table names
// the set's own arrays and b comes from the set's records; only those two segments have items.
// With a pack that holds a walk plan (its counters' kCntPlanReady, read here: one capture serves packs
// with and without), the table also names the pack's cover masks.
__global__ __launch_bounds__(kViewThreads) void k_view_bind(ViewCopy p, float4* plane, ViewBind* bind, int identity)
{
    const size_t stride = (size_t)gridDim.x * kViewThreads;
    const bool plan = !identity && p.plan_room && p.pk_counters[kCntPlanReady] != 0u;
    for (size_t i = (size_t)blockIdx.x * kViewThreads + threadIdx.x; i < p.end[kSegs - 1]; i += stride) {
        if (i < p.end[kSegRecord]) {  // .x only: the language slots .yzw belong to the feature fill
            const float b = identity ? reinterpret_cast<const float*>(p.record + 3 * i + 2)[0] : p.pk_recb[i];
            reinterpret_cast<float*>(plane + i)[0] = b;
        } else if (i < p.end[kSegPointList]) {
            ViewBind t{};
            if (plan) {
                t.cover = reinterpret_cast<const uint8_t*>(p.pk_cover);
                t.plan = kPlanOn;
            }
            t.rec01 = identity ? p.record : p.pk_rec01;
            t.s01 = identity ? 3u : 2u;
            t.recb = plane;
            t.sb = 1u;
            t.point_list = reinterpret_cast<const uint32_t*>(identity ? p.point_list : p.pk_point_list);
            *bind = t;
        } else if (i < p.end[kSegRadii]) {
            move_radii<true>(p, i - p.end[kSegPointList]);
        } else if (i < p.end[kSegClamped]) {
            move<true>(p.clamped, p.pk_clamped, i - p.end[kSegRadii]);
        } else if (i < p.end[kSegRanges]) {
            move<true>(p.ranges, p.pk_ranges, i - p.end[kSegClamped]);
        } else if (i < p.end[kSegOrder]) {
            move_order<true>(p, (uint32_t)(i - p.end[kSegRanges]));
        } else if (i < p.end[kSegCounters]) {
            restore_counter(p, (int)(i - p.end[kSegOrder]));
        } else {
            p.loss_words[i - p.end[kSegCounters]] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
}

__global__ __launch_bounds__(64) void k_view_counts(const uint32_t* __restrict__ counters, uint32_t* host)
{
    if (threadIdx.x < 8)
        __hip_atomic_store(&host[threadIdx.x], counters[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

hipError_t launch_view_counts(const uint32_t* counters, uint32_t* host, hipStream_t s)
{
    hipLaunchKernelGGL(k_view_counts, dim3(1), dim3(64), 0, s, counters, host);
    return hipGetLastError();
}

static ViewCopy view_copy_params(const ViewParams& v, const Layout& L)
{
    const ViewPack V = make_view_pack(v.P, v.W, v.H, v.R);
    ViewCopy p{};
    p.P = v.P;
    p.T = L.tiles;
    p.R = v.R;
    p.radii_vec = (reinterpret_cast<uintptr_t>(v.radii) & 15) == 0 ? 1 : 0;
    p.fwd_flags = v.fwd_flags;
    p.record = reinterpret_cast<float4*>(v.geom + L.record);
    p.radii = v.radii;
    p.clamped = reinterpret_cast<uint4*>(v.geom + L.clamped);
    p.ranges = reinterpret_cast<uint4*>(v.image + L.ranges);
    p.lists = reinterpret_cast<uint32_t*>(v.image + L.tile_lists);
    p.point_list = reinterpret_cast<uint4*>(v.binning + L.point_list);
    p.counters = reinterpret_cast<uint32_t*>(v.image + L.counters);
    p.loss_words = reinterpret_cast<uint4*>(v.geom + L.loss_words);
    p.overflow = v.overflow;
    p.pk_counters = reinterpret_cast<uint32_t*>(v.pack + V.counters);
    p.pk_rec01 = reinterpret_cast<float4*>(v.pack + V.rec01);
    p.pk_recb = reinterpret_cast<float*>(v.pack + V.recb);
    p.pk_radii = reinterpret_cast<int32_t*>(v.pack + V.radii);
    p.pk_clamped = reinterpret_cast<uint4*>(v.pack + V.clamped);
    p.pk_ranges = reinterpret_cast<uint4*>(v.pack + V.ranges);
    p.pk_order = reinterpret_cast<uint32_t*>(v.pack + V.order);
    p.pk_point_list = reinterpret_cast<uint4*>(v.pack + V.point_list);
    p.cover = reinterpret_cast<uint4*>(v.binning + L.cover);
    p.pk_cover = reinterpret_cast<uint4*>(v.pack + V.cover);
    p.plan_room = v.plan_room ? 1 : 0;
    return p;
}

static dim3 view_grid(size_t n)
{
    const size_t blocks = (n + kViewThreads - 1) / kViewThreads;
    return dim3((unsigned)(blocks < (size_t)kViewMaxBlocks ? blocks : (size_t)kViewMaxBlocks));
}

hipError_t launch_view_copy(const ViewParams& v, bool restore, hipStream_t s)
{
    const Layout L = make_layout(v.P, v.W, v.H, v.R_cap, 0);  // point_list sits at offset 0
    ViewCopy p = view_copy_params(v, L);
    const size_t P = (size_t)v.P, T = (size_t)L.tiles, R = (size_t)v.R;
    size_t n = 0;
    p.end[kSegRecord] = n += 3 * P;
    p.end[kSegPointList] = n += (R + 3) / 4;
    p.end[kSegRadii] = n += (P + 3) / 4;
    p.end[kSegClamped] = n += (P + 3) / 4;
    p.end[kSegRanges] = n += (T + 1) / 2;
    p.end[kSegOrder] = n += T;
    p.end[kSegCounters] = n += restore ? (size_t)kCntWords : (size_t)kViewCounterWords;
    p.end[kSegLoss] = n += restore ? (T + 1) / 2 : 0;
    // (the array is padded past a whole number of 16-byte words, in the set and in the pack)
    p.end[kSegCover] = n += !restore && v.plan_room ? (R + 15) / 16 : 0;
    const dim3 grid = view_grid(n);
    if (restore)
        hipLaunchKernelGGL(k_view_copy<true>, grid, dim3(kViewThreads), 0, s, p);
    else
        hipLaunchKernelGGL(k_view_copy<false>, grid, dim3(kViewThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_view_bind(const ViewParams& v, bool clamped, hipStream_t s)
{
    const Layout L = make_layout(v.P, v.W, v.H, v.R_cap, 0);
    const bool identity = v.pack == nullptr;
    ViewParams vv = v;
    if (identity) vv.R = 0;  // (no pack offset is used)
    ViewCopy p = view_copy_params(vv, L);
    const size_t P = (size_t)v.P, T = (size_t)L.tiles;
    size_t n = 0;
    p.end[kSegRecord] = n += P;
    p.end[kSegPointList] = n += 1;
    p.end[kSegRadii] = n += identity ? 0 : (P + 3) / 4;
    p.end[kSegClamped] = n += identity || !clamped ? 0 : (P + 3) / 4;
    p.end[kSegRanges] = n += identity ? 0 : (T + 1) / 2;
    p.end[kSegOrder] = n += identity ? 0 : T;
    p.end[kSegCounters] = n += identity ? 0 : (size_t)kCntWords;
    p.end[kSegLoss] = n += identity ? 0 : (T + 1) / 2;
    p.end[kSegCover] = n;
    hipLaunchKernelGGL(k_view_bind, view_grid(n), dim3(kViewThreads), 0, s, p, reinterpret_cast<float4*>(v.geom + L.lang_plane),
                       reinterpret_cast<ViewBind*>(v.geom + L.view_bind), identity ? 1 : 0);
    return hipGetLastError();
}

}  // namespace lsr
