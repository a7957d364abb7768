// lsr_eval.hip -- LERF evaluation after get_max_across: the 30 x 30 mean filter, the blend and its
// statistics (lsr_eval_filter), then the thresholded and majority-smoothed masks with their
// intersection / union counts (lsr_eval_masks); include/lsr.h has the semantics.
//
// Reference op sequence: eval/evaluate_iou_loc.py:107-112 and :176-187 (cv2.filter2D with a 30 x 30 mean
// kernel, 0.5 * (avg + map), the maxima), :129-143 (normalise by the map's own min / max, clip,
// threshold, smooth(), intersection and union) and eval/utils.py:46-55 (smooth()).
//
// Both kernels give a workgroup of 4 waves a tile of kETh x kETw = 32 x 64 outputs of one map.
//   k_eval_filter: the tile plus its 29-sample halo (61 x 93 floats, reflected at the borders) is
//     staged in LDS once.  Pass 1 sums 30 taps along x for the 61 rows into hs[61][64]; pass 2 sums
//     30 rows of hs along y.  In both passes a thread reads 33 consecutive samples into registers
//     and forms 4 adjacent outputs from them, each as its own fixed-order sum of 30 taps (three
//     chains of 10, then (a + b) + c): 8.25 LDS reads per output and pass instead of 30, and no
//     sliding window.  Pass 1 puts consecutive ROWS on consecutive lanes (row strides 93 and 65
//     floats, both odd: 32 lanes on 32 banks), pass 2 consecutive columns.
//     LDS: 4 (61 * 93 + 61 * 65) = 38.6 KB, 4 workgroups per CU.
//   k_eval_masks: the raw mask of the tile plus a 3-pixel halo (38 x 70) is recomputed from blend
//     into LDS (zero outside the image), then 7 taps along x and 7 along y count the window's ones;
//     smooth()'s exclusive upper bound clipped to H - 1 / W - 1 is a predicate on the tap's row / column.
//   k_label_stats (lsr_label_stats): per-class counts of predicted against ground-truth labels, LDS
//     counters per workgroup and one integer atomic per non-zero counter (see the kernel).
// Statistics and counts: wave shuffles, 4 partials through LDS, then one integer atomic per
// workgroup and value (min / max of order-preserving keys, add of counts): the result does not
// depend on the order, so two runs are bit-identical.
#include "lsr_internal.h"

namespace lsr {
namespace {

constexpr int kEThreads = 256;
constexpr int kEWaves = kEThreads / 64;
constexpr int kETh = 32, kETw = 64;          // outputs per workgroup
constexpr int kEK = 30, kEAnchor = 15;       // taps -15 .. +14
constexpr int kEHaloH = kETh + kEK - 1;      // 61
constexpr int kEHaloW = kETw + kEK - 1;      // 93: the staged tile's row stride (odd)
constexpr int kEHs = kETw + 1;               // 65: row stride of the row sums (odd)
constexpr int kESeg = 4;                     // adjacent outputs per thread and pass
constexpr int kEMaxGridY = 65535;
constexpr int kSm = 3;                       // smooth()'s scale: rows i - 3 .. i + 3
constexpr int kSmH = kETh + 2 * kSm;         // 38
constexpr int kSmW = kETw + 2 * kSm;         // 70
constexpr int kSmRaw = 72;                   // row stride of the raw mask bytes
static_assert(kETw == 64 && kEThreads == 4 * 64 && kETh % (kEWaves * kESeg) == 0 && kETw % kESeg == 0, "tile plan");

// BORDER_REFLECT_101 with period 2 (n - 1), n >= 2: gfedcb|abcdefgh|gfedcba
// The pattern is symmetric about 0 and about n - 1, so one reflection at each end settles every index
// within n - 1 of the map without a division; the rest (a map narrower than the halo) takes the modulo.
__device__ __forceinline__ int reflect101(int i, int n)
{
    const int p = 2 * (n - 1);
    if (i < 0) i = -i;
    if (i >= n) i = p - i;
    if ((unsigned)i >= (unsigned)n) {
        i %= p;
        if (i < 0) i += p;
        i = i >= n ? p - i : i;
    }
    return i;
}

// order-preserving map of a float onto unsigned integers (-0 below +0) and back
__device__ __forceinline__ uint32_t ordered_key(float v)
{
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ordered_value(uint32_t k)
{
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// taps K .. K + 29 of v: three chains of 10 consecutive taps, then (a + b) + c
template <int K>
__device__ __forceinline__ float sum30(const float (&v)[kEK + kESeg - 1])
{
    float a = v[K], b = v[K + 10], c = v[K + 20];
#pragma unroll
    for (int t = 1; t < 10; t++) {
        a += v[K + t];
        b += v[K + 10 + t];
        c += v[K + 20 + t];
    }
    return (a + b) + c;
}

// A record while lsr_eval_filter's kernels run: word 0 the smallest key of blend, word 1 the largest,
// words 2-3 one 64-bit value, (key of avg) << 32 | ~index, the largest of which is the maximum of avg
// at its first index.
__global__ void k_eval_stats_init(uint32_t* rec, int n_maps)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m < n_maps) {
        rec[4 * m] = 0xFFFFFFFFu;
        rec[4 * m + 1] = 0u;
        rec[4 * m + 2] = 0u;
        rec[4 * m + 3] = 0u;
    }
}

__global__ void k_eval_stats_final(uint32_t* rec, int n_maps)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m < n_maps) {
        const uint32_t kmin = rec[4 * m], kmax = rec[4 * m + 1], nidx = rec[4 * m + 2], kavg = rec[4 * m + 3];
        lsr_eval_stats s;
        s.blend_min = ordered_value(kmin);
        s.blend_max = ordered_value(kmax);
        s.avg_max = ordered_value(kavg);
        s.avg_argmax = (int32_t)~nidx;
        reinterpret_cast<lsr_eval_stats*>(rec)[m] = s;
    }
}

__global__ __launch_bounds__(kEThreads) void k_eval_filter(const lsr_eval_filter_args p, int map0)
{
    __shared__ float tile[kEHaloH * kEHaloW];
    __shared__ float hs[kEHaloH * kEHs];
    __shared__ uint32_t r_min[kEWaves], r_max[kEWaves];
    __shared__ unsigned long long r_arg[kEWaves];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: row work is scalar
    const int H = p.H, W = p.W;
    const int tiles_x = (W + kETw - 1) / kETw;
    const int ty0 = (int)(blockIdx.x / tiles_x) * kETh, tx0 = (int)(blockIdx.x % tiles_x) * kETw;
    const int m = map0 + (int)blockIdx.y;
    const size_t base = (size_t)m * (size_t)H * (size_t)W;
    const float* src = p.maps + base;

    {  // the tile and its halo, reflected into the map: every read is inside it.  A wave takes rows
       // w, w + 4, ... (the rows' reflections are computed once, one per lane, and broadcast), a lane
       // columns lane and lane + 64 (past the halo: column 92 again, the same value to the same place).
       // All of a thread's loads are issued before the first LDS store waits for one: a loop that
       // loads and stores row by row pays the memory latency once per row.
        constexpr int kRows = (kEHaloH + kEWaves - 1) / kEWaves;  // 16
        const int c1 = lane + 64;
        const int gx0 = reflect101(tx0 - kEAnchor + lane, W);
        const int gx1 = reflect101(tx0 - kEAnchor + min(c1, kEHaloW - 1), W);
        const int gy = reflect101(ty0 - kEAnchor + min(lane, kEHaloH - 1), H);  // lane r: staged row r's row of the map
        float v0[kRows], v1[kRows];
#pragma unroll
        for (int k = 0; k < kRows; k++) {
            const int r = min(w + k * kEWaves, kEHaloH - 1);  // the last wave-rows repeat row 60
            const float* row = src + (size_t)__builtin_amdgcn_readlane(gy, r) * W;
            v0[k] = row[gx0];
            v1[k] = row[gx1];
        }
#pragma unroll
        for (int k = 0; k < kRows; k++) {
            const int r = min(w + k * kEWaves, kEHaloH - 1);
            tile[r * kEHaloW + lane] = v0[k];
            tile[r * kEHaloW + min(c1, kEHaloW - 1)] = v1[k];
        }
    }
    __syncthreads();

    // pass 1: hs[r][x] = taps x .. x + 29 of row r
    for (int i = tid; i < kEHaloH * (kETw / kESeg); i += kEThreads) {
        const int seg = i / kEHaloH, r = i - seg * kEHaloH, x0 = seg * kESeg;
        float v[kEK + kESeg - 1];
        const float* in = tile + r * kEHaloW + x0;
#pragma unroll
        for (int t = 0; t < kEK + kESeg - 1; t++) v[t] = in[t];
        float* o = hs + r * kEHs + x0;
        o[0] = sum30<0>(v);
        o[1] = sum30<1>(v);
        o[2] = sum30<2>(v);
        o[3] = sum30<3>(v);
    }
    __syncthreads();

    // pass 2: rows y .. y + 29 of hs, the scale, the blend and the statistics
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
    unsigned long long karg = 0ull;
    const int gx = tx0 + lane;
#pragma unroll 1
    for (int yb = w * kESeg; yb < kETh; yb += kEWaves * kESeg) {
        float v[kEK + kESeg - 1];
#pragma unroll
        for (int t = 0; t < kEK + kESeg - 1; t++) v[t] = hs[(yb + t) * kEHs + lane];
        const float s[kESeg] = {sum30<0>(v), sum30<1>(v), sum30<2>(v), sum30<3>(v)};
#pragma unroll
        for (int k = 0; k < kESeg; k++) {
            const int gy = ty0 + yb + k;
            if (gy < H && gx < W) {
                const float avg = s[k] / 900.0f;
                const float blend = 0.5f * (avg + tile[(yb + k + kEAnchor) * kEHaloW + lane + kEAnchor]);
                const uint32_t idx = (uint32_t)gy * (uint32_t)W + (uint32_t)gx;
                if (p.out_avg) p.out_avg[base + idx] = avg;
                if (p.out_blend) p.out_blend[base + idx] = blend;
                const uint32_t kb = ordered_key(blend);
                kmin = kb < kmin ? kb : kmin;
                kmax = kb > kmax ? kb : kmax;
                const unsigned long long ka = ((unsigned long long)ordered_key(avg) << 32) | (uint32_t)~idx;
                karg = ka > karg ? ka : karg;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t omin = __shfl_xor(kmin, off), omax = __shfl_xor(kmax, off);
        const unsigned long long oarg = __shfl_xor(karg, off);
        kmin = omin < kmin ? omin : kmin;
        kmax = omax > kmax ? omax : kmax;
        karg = oarg > karg ? oarg : karg;
    }
    if (lane == 0) {
        r_min[w] = kmin;
        r_max[w] = kmax;
        r_arg[w] = karg;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int i = 1; i < kEWaves; i++) {
            kmin = r_min[i] < kmin ? r_min[i] : kmin;
            kmax = r_max[i] > kmax ? r_max[i] : kmax;
            karg = r_arg[i] > karg ? r_arg[i] : karg;
        }
        // a tile wholly inside the map's padding (none exists: the grid covers the map) would add nothing
        uint32_t* rec = reinterpret_cast<uint32_t*>(p.out_stats + m);
        atomicMin(rec, kmin);
        atomicMax(rec + 1, kmax);
        atomicMax(reinterpret_cast<unsigned long long*>(rec + 2), karg);
    }
}

__global__ __launch_bounds__(kEThreads) void k_eval_masks(const lsr_eval_mask_args p, int map0)
{
    __shared__ uint8_t raw[kSmH * kSmRaw];
    __shared__ int hc[kSmH * kEHs];
    __shared__ int r_cnt[2 * kEWaves];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: row work is scalar
    const int H = p.H, W = p.W;
    const int tiles_x = (W + kETw - 1) / kETw;
    const int ty0 = (int)(blockIdx.x / tiles_x) * kETh, tx0 = (int)(blockIdx.x % tiles_x) * kETw;
    const int m = map0 + (int)blockIdx.y;
    const size_t base = (size_t)m * (size_t)H * (size_t)W;
    const float* src = p.blend + base;
    const float mn = p.stats[m].blend_min, mx = p.stats[m].blend_max;
    const float den = (mx - mn) + 1e-9f;

    // the raw mask of the tile and 3 pixels around it; outside the map it is 0 (never inside a window).
    // Every load is issued before the first result is used: the addresses are clamped into the map
    // and the value outside it discarded (also for the ground truth of the thread's 8 output rows).
    constexpr int kItems = (kSmH * kSmW + kEThreads - 1) / kEThreads;  // 11
    constexpr int kRows = kETh / kEWaves;                              // 8
    const int gx = tx0 + lane;
    const uint8_t* gt = p.gt_mask ? p.gt_mask + (size_t)(m % p.n_prompts) * (size_t)H * (size_t)W : nullptr;
    float xv[kItems];
    int gv[kRows] = {};
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        const int i = min(tid + k * kEThreads, kSmH * kSmW - 1);
        const int r = i / kSmW, c = i - r * kSmW;
        const int y = min(max(ty0 - kSm + r, 0), H - 1), x = min(max(tx0 - kSm + c, 0), W - 1);
        xv[k] = src[(size_t)y * W + x];
    }
    if (gt) {
#pragma unroll
        for (int k = 0; k < kRows; k++) gv[k] = gt[(size_t)min(ty0 + w + k * kEWaves, H - 1) * W + min(gx, W - 1)];
    }
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        const int i = tid + k * kEThreads;
        const int r = i / kSmW, c = i - r * kSmW;
        const int y = ty0 - kSm + r, x = tx0 - kSm + c;
        if (i < kSmH * kSmW) {
            uint8_t v = 0;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                float o = xv[k] - mn;
                o = o / den;
                o = o * 2.0f + (-1.0f);
                o = fminf(fmaxf(o, 0.0f), 1.0f);
                v = o > p.thresh ? 1 : 0;
                if (p.out_mask_raw && r >= kSm && r < kSm + kETh && c >= kSm && c < kSm + kETw)
                    p.out_mask_raw[base + (size_t)y * W + x] = v;
            }
            raw[r * kSmRaw + c] = v;
        }
    }
    __syncthreads();

    // ones in columns max(0, x - 3) .. min(x + 4, W - 1) - 1 of each staged row: the columns left of
    // the map hold zeros, a column from W - 1 on is outside every window
    for (int r = w; r < kSmH; r += kEWaves) {
        int n = 0;
#pragma unroll
        for (int d = 0; d < 2 * kSm + 1; d++) n += (gx - kSm + d < W - 1) ? raw[r * kSmRaw + lane + d] : 0;
        hc[r * kEHs + lane] = n;
    }
    __syncthreads();

    const int c0 = max(0, gx - kSm), c1 = min(gx + kSm + 1, W - 1);
    int inter = 0, uni = 0;
#pragma unroll
    for (int k = 0; k < kRows; k++) {
        const int yy = w + k * kEWaves, gy = ty0 + yy;
        if (gy < H && gx < W) {
            int ones = 0;
#pragma unroll
            for (int d = 0; d < 2 * kSm + 1; d++) ones += (gy - kSm + d < H - 1) ? hc[(yy + d) * kEHs + lane] : 0;
            const int r0 = max(0, gy - kSm), r1 = min(gy + kSm + 1, H - 1);
            const int size = (r1 - r0) * (c1 - c0);
            const int s = 2 * ones > size ? 1 : 0;
            p.out_mask[base + (size_t)gy * W + gx] = (uint8_t)s;
            const int g = gv[k] != 0 ? 1 : 0;  // 0 without a ground truth
            inter += g & s;
            uni += g | s;
        }
    }
    if (gt) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            inter += __shfl_xor(inter, off);
            uni += __shfl_xor(uni, off);
        }
        if (lane == 0) {
            r_cnt[2 * w] = inter;
            r_cnt[2 * w + 1] = uni;
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int i = 1; i < kEWaves; i++) {
                inter += r_cnt[2 * i];
                uni += r_cnt[2 * i + 1];
            }
            unsigned long long* cnt = reinterpret_cast<unsigned long long*>(p.out_counts) + 2 * (size_t)m;
            if (inter) atomicAdd(cnt, (unsigned long long)inter);
            if (uni) atomicAdd(cnt + 1, (unsigned long long)uni);
        }
    }
}

// lsr_label_stats: per-class counts of a predicted against a ground-truth label map.  A workgroup
// takes kLSweep = 2048 consecutive pixels of one map per sweep (grid-stride over the map: more than
// one sweep only past kLMaxBlocks * kLSweep pixels).  Every load of a sweep is issued before the first
// LDS update waits for one (addresses clamped into the map, the value past it discarded).  Counters
// live in LDS as 32-bit integers (a workgroup sees fewer than 2^32 pixels: launch_label_stats' bound on
// N); only the non-zero ones are flushed, one 64-bit integer atomic each.  Integer adds commute, so the
// result is exact and two calls are identical.
constexpr int kLItems = 8;
constexpr int kLSweep = kEThreads * kLItems;  // 2048
constexpr int kLMaxBlocks = 1024;
constexpr int kLMaxClasses = 64;

__global__ __launch_bounds__(kEThreads) void k_label_stats(const lsr_label_stats_args p, int map0)
{
    __shared__ unsigned int cnt[kLMaxClasses * 3];  // per class: intersection, predicted, ground truth
    __shared__ unsigned int tot[2];                 // correct, valid
    const int tid = threadIdx.x;
    const int m = map0 + (int)blockIdx.y;
    const int C = p.n_classes;
    const int32_t* pred = p.pred + (size_t)m * (size_t)p.N;
    const int32_t* gt = p.gt + (p.gt_maps == 1 ? (size_t)0 : (size_t)m * (size_t)p.N);
    for (int i = tid; i < 3 * C; i += kEThreads) cnt[i] = 0u;
    if (tid < 2) tot[tid] = 0u;
    __syncthreads();
    for (int64_t base = (int64_t)blockIdx.x * kLSweep; base < p.N; base += (int64_t)gridDim.x * kLSweep) {
        int pv[kLItems], gv[kLItems];
#pragma unroll
        for (int k = 0; k < kLItems; k++) {
            const int64_t i = base + k * kEThreads + tid;
            const int64_t ic = i < p.N ? i : p.N - 1;
            pv[k] = pred[ic];
            gv[k] = gt[ic];
        }
#pragma unroll
        for (int k = 0; k < kLItems; k++) {
            const int g = gv[k], q = pv[k];
            if (base + k * kEThreads + tid < p.N && (unsigned)g < (unsigned)C) {
                atomicAdd(&cnt[3 * g + 2], 1u);
                if ((unsigned)q < (unsigned)C) atomicAdd(&cnt[3 * q + 1], 1u);
                if (q == g) atomicAdd(&cnt[3 * g], 1u);
            }
        }
    }
    __syncthreads();
    // correct = sum of the intersections, valid = sum of the ground-truth counts
    if (tid < C) {
        if (cnt[3 * tid]) atomicAdd(&tot[0], cnt[3 * tid]);
        if (cnt[3 * tid + 2]) atomicAdd(&tot[1], cnt[3 * tid + 2]);
    }
    unsigned long long* oc = reinterpret_cast<unsigned long long*>(p.out_counts) + (size_t)m * 3 * (size_t)C;
    for (int i = tid; i < 3 * C; i += kEThreads)
        if (cnt[i]) atomicAdd(oc + i, (unsigned long long)cnt[i]);
    __syncthreads();
    if (tid < 2 && tot[tid]) atomicAdd(reinterpret_cast<unsigned long long*>(p.out_totals) + 2 * (size_t)m + tid, (unsigned long long)tot[tid]);
}

unsigned eval_tiles(int H, int W)
{
    return (unsigned)(((H + kETh - 1) / kETh) * ((W + kETw - 1) / kETw));  // H W < 2^31: fewer than 2^20 tiles
}

}  // namespace

hipError_t launch_eval_filter(const lsr_eval_filter_args& a, hipStream_t s)
{
    if (a.n_maps == 0) return hipSuccess;
    uint32_t* rec = reinterpret_cast<uint32_t*>(a.out_stats);
    const unsigned small = (unsigned)((a.n_maps + 255) / 256);
    hipLaunchKernelGGL(k_eval_stats_init, dim3(small), dim3(256), 0, s, rec, a.n_maps);
    for (int map0 = 0; map0 < a.n_maps; map0 += kEMaxGridY) {
        const int n = a.n_maps - map0 < kEMaxGridY ? a.n_maps - map0 : kEMaxGridY;
        hipLaunchKernelGGL(k_eval_filter, dim3(eval_tiles(a.H, a.W), (unsigned)n), dim3(kEThreads), 0, s, a, map0);
    }
    hipLaunchKernelGGL(k_eval_stats_final, dim3(small), dim3(256), 0, s, rec, a.n_maps);
    return hipGetLastError();
}

hipError_t launch_eval_masks(const lsr_eval_mask_args& a, hipStream_t s)
{
    if (a.n_maps == 0) return hipSuccess;
    if (a.gt_mask) {
        const hipError_t e = hipMemsetAsync(a.out_counts, 0, 2 * sizeof(int64_t) * (size_t)a.n_maps, s);
        if (e != hipSuccess) return e;
    }
    for (int map0 = 0; map0 < a.n_maps; map0 += kEMaxGridY) {
        const int n = a.n_maps - map0 < kEMaxGridY ? a.n_maps - map0 : kEMaxGridY;
        hipLaunchKernelGGL(k_eval_masks, dim3(eval_tiles(a.H, a.W), (unsigned)n), dim3(kEThreads), 0, s, a, map0);
    }
    return hipGetLastError();
}

hipError_t launch_label_stats(const lsr_label_stats_args& a, hipStream_t s)
{
    if (a.n_maps == 0 || a.N == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(a.out_counts, 0, 3 * sizeof(int64_t) * (size_t)a.n_maps * (size_t)a.n_classes, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(a.out_totals, 0, 2 * sizeof(int64_t) * (size_t)a.n_maps, s);
    if (e != hipSuccess) return e;
    const int64_t sweeps = (a.N + kLSweep - 1) / kLSweep;
    const unsigned blocks = (unsigned)(sweeps < kLMaxBlocks ? sweeps : kLMaxBlocks);
    for (int map0 = 0; map0 < a.n_maps; map0 += kEMaxGridY) {
        const int n = a.n_maps - map0 < kEMaxGridY ? a.n_maps - map0 : kEMaxGridY;
        hipLaunchKernelGGL(k_label_stats, dim3(blocks, (unsigned)n), dim3(kEThreads), 0, s, a, map0);
    }
    return hipGetLastError();
}

}  // namespace lsr
