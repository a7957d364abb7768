// lsr_query.hip -- open-vocabulary query: the autoencoder's decoder MLP, the L2 normalisation, the
// phrase similarities and the relevancy in ONE kernel (lsr_query_relevancy, include/lsr.h).
//
// Reference op sequence (eval/evaluate_iou_loc.py:258-266): Autoencoder.decode
// (autoencoder/model.py:42-46: Linear, [ReLU, Linear]*, x / ||x||) then
// OpenCLIPNetwork.get_max_across / get_relevancy (eval/openclip_encoder.py:42-56, 96-112).
//
// One workgroup (8 waves, 2 per SIMD) owns kQPix = 64 pixels.  Every product is computed TRANSPOSED on the exact
// fp32 MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain):
//     Y^T[out, px] = W[out, in] . H^T[in, px]        A = W (staged in LDS), B = H^T (LDS), C = bias
// so an accumulator tile has the PIXEL on the lane and 32 output features in its 16 registers x 2
// lane halves (row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)).  A wave owns the 32-feature tiles
// w and w + 8 of a layer for both 32-pixel halves: up to 4 independent accumulators.
//   - activations: LDS image act[feature][64 px] (the two pixel halves swapped on odd rows, so the
//     two lane halves of a B read hit different banks).  A layer's outputs stay in registers until
//     every wave has read the inputs, then overwrite them in place (ReLU applied at the store).
//   - weights: nn.Linear's W (out x in, row-major) is read from L2 in chunks of kc input columns,
//     transposed on the way into LDS (wl[k][out]); the next chunk's global loads are in flight
//     while the current one feeds the MFMAs (two LDS buffers, one barrier per chunk).
//   - last layer: its tiles never leave the registers.  A tile is the B operand of the phrase
//     product as it stands (accumulator-as-operand: S^T[phrase, px] += P[phrase, d] . Y^T[d, px], the
//     k order permuted to the accumulator's row order and the phrase operand read to match), and
//     its squares go into the pixel's ||y||^2.
//   - epilogue: the waves' partial similarities and norms are summed through LDS in a fixed order,
//     then r[j, px] = 1 / (1 + exp(10 (max_n s_n - s_j))): the minimum over the negatives of a
//     function that decreases in s_n is its value at the largest s_n.
// No atomics; every sum has a fixed order, so two runs are bit-identical.
// k_query_semantic (lsr_query_semantic) is the same body with another epilogue: a label and its
// softmax value per pixel instead of the relevancies (see the kernel).
#include <mutex>

#include "lsr_internal.h"

namespace lsr {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kQThreads = 512;
constexpr int kQWaves = kQThreads / 64;  // 2 per SIMD: one wave's LDS waits and staging hide behind the other's MFMAs
constexpr int kQTiles = 2;       // 32-feature tiles per wave and layer (8 waves x 2 x 32 = 512 features)
constexpr int kQStage = 4;       // staged float4s per thread and chunk: 16 rows x 512 columns / 4 / 512

// feature row of accumulator register r in lane half h (the 32x32 MFMA's C/D map)
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

struct LayerDims {
    int k_in;       // contraction length (the 3 input features are padded to 4)
    int n_out;      // output features
    int tiles;      // 32-feature tiles
    const float* W;
    const float* b;
};

__device__ __forceinline__ LayerDims layer_dims(const QueryParams& p, int l)
{
    LayerDims d;
    d.k_in = l ? p.widths[l - 1] : 4;
    d.n_out = p.widths[l];
    d.tiles = (d.n_out + 31) >> 5;
    d.W = p.weights + p.w_off[l];
    d.b = d.W + (size_t)d.n_out * (size_t)(l ? d.k_in : 3);
    return d;
}

// A thread's share of a layer's weight staging, the same for every chunk of the layer (a layer's
// chunks all have `rows` = min(kc, k_in) input columns: k_in is 4 or a multiple of 16, kc 4, 8 or 16).
// Item i is float4 (idx % r4) of column (idx / r4), idx = tid + i * kQThreads, r4 = rows / 4: the lanes
// of a load cover whole 16..64-byte runs of W's rows.  Columns past n_out (a width of 16 mod 32)
// stage zeros.
struct StagePlan {
    const float* src[kQStage];  // the item's float4 in chunk 0; null: zeros
    int dst[kQStage];           // its first float in a staging buffer (wl[4 q4][col]); -1: no item
};

__device__ __forceinline__ StagePlan stage_plan(const LayerDims& d, int l, int rows, int tid, int ws)
{
    const int lg = rows >> 3 ? (rows >> 4 ? 2 : 1) : 0;  // rows 4 / 8 / 16 -> float4s per column 1 / 2 / 4
    const int total = (d.tiles * 32) << lg;
    const int stride = l ? d.k_in : 3;  // floats per row of W
    StagePlan sp;
#pragma unroll
    for (int i = 0; i < kQStage; i++) {
        const int idx = tid + i * kQThreads;
        const int col = idx >> lg, q4 = idx & ((1 << lg) - 1);
        sp.dst[i] = idx < total ? 4 * q4 * ws + col : -1;
        sp.src[i] = idx < total && col < d.n_out ? d.W + (size_t)col * stride + 4 * q4 : nullptr;
    }
    return sp;
}

// global -> registers; layer 0's rows have 3 floats (scalar loads, one chunk)
__device__ __forceinline__ void stage_load(const StagePlan& sp, int l, int k0, float4 (&v)[kQStage])
{
#pragma unroll
    for (int i = 0; i < kQStage; i++) {
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (sp.src[i]) {
            if (l) v[i] = *reinterpret_cast<const float4*>(sp.src[i] + k0);
            else v[i] = make_float4(sp.src[i][0], sp.src[i][1], sp.src[i][2], 0.f);
        }
    }
}

// registers -> LDS, transposed: wl[k][column]
__device__ __forceinline__ void stage_store(const StagePlan& sp, int ws, float* wb, const float4 (&v)[kQStage])
{
#pragma unroll
    for (int i = 0; i < kQStage; i++) {
        if (sp.dst[i] >= 0) {
            float* o = wb + sp.dst[i];
            o[0] = v[i].x;
            o[ws] = v[i].y;
            o[2 * ws] = v[i].z;
            o[3 * ws] = v[i].w;
        }
    }
}

// operands of one pair of k steps for the wave's NQ tiles
template <int NQ>
struct PairOps {
    float b00, b01, b10, b11, a0[NQ], a1[NQ];
};
template <int NQ>
__device__ __forceinline__ PairOps<NQ> pair_load(const float* a_k, const float* w_k, int ws, int b0_off, int b1_off)
{
    PairOps<NQ> o;
    o.b00 = a_k[b0_off];
    o.b01 = a_k[b1_off];
    o.b10 = a_k[128 + b0_off];
    o.b11 = a_k[128 + b1_off];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        o.a0[q] = w_k[q * 32 * kQWaves];
        o.a1[q] = w_k[2 * ws + q * 32 * kQWaves];
    }
    return o;
}

// one staged chunk into the wave's NQ tiles: `pairs` pairs of k steps (a chunk has a multiple of 4
// rows); a_k / w_k point at this lane's first B row and A row.  The next pair's operands are read
// from LDS before the current pair's MFMAs issue.
template <int NQ>
__device__ __forceinline__ void chunk_mma(const float* a_k, const float* w_k, int ws, int pairs, int b0_off, int b1_off,
                                          f32x16 (&acc)[kQTiles][2])
{
    PairOps<NQ> cur = pair_load<NQ>(a_k, w_k, ws, b0_off, b1_off);
    for (int s = 0; s < pairs; s++) {
        PairOps<NQ> nxt = cur;
        if (s + 1 < pairs) {
            a_k += 256;
            w_k += 4 * ws;
            nxt = pair_load<NQ>(a_k, w_k, ws, b0_off, b1_off);
        }
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            acc[q][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a0[q], cur.b00, acc[q][0], 0, 0, 0);
            acc[q][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a0[q], cur.b01, acc[q][1], 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            acc[q][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a1[q], cur.b10, acc[q][0], 0, 0, 0);
            acc[q][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a1[q], cur.b11, acc[q][1], 0, 0, 0);
        }
        cur = nxt;
    }
}

// every chunk of layer l: stage chunk c + 1 (global loads before, LDS stores after the MFMAs of chunk
// c), one barrier per chunk
template <int NQ>
__device__ __forceinline__ void chunk_loop(const QueryParams& p, const LayerDims& d, int l, int w, const float* act,
                                           float* wl, f32x16 (&acc)[kQTiles][2])
{
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int kc = p.kc, ws = p.ws;
    const int rows = d.k_in < kc ? d.k_in : kc;
    const int chunks = d.k_in / rows;
    const StagePlan sp = stage_plan(d, l, rows, tid, ws);
    float4 v[kQStage];
    stage_load(sp, l, 0, v);
    stage_store(sp, ws, wl, v);
    __syncthreads();  // the staged chunk, and the activations the previous layer stored
    // B reads: row k has parity h (k0 and 2 s are even), so lane half h finds pixel half 0 at j + 32 h
    const int b0_off = j ^ (h << 5), b1_off = (32 + j) ^ (h << 5);
    const float* a_k = act + h * 64;
    const float* w_k = wl + h * ws + w * 32 + j;
    for (int c = 0; c < chunks; c++) {
        const bool more = c + 1 < chunks;
        if (more) stage_load(sp, l, (c + 1) * rows, v);
        if (NQ > 0)
            chunk_mma<(NQ > 0 ? NQ : 1)>(a_k + c * rows * 64, w_k + (c & 1) * kc * ws, ws, rows >> 2, b0_off, b1_off, acc);
        if (more) stage_store(sp, ws, wl + ((c + 1) & 1) * kc * ws, v);
        __syncthreads();
    }
}

// acc[q][half] = bias + W . H^T for the wave's tiles of layer l; act and wl as described above.
// Ends with a barrier after the last read of act and wl.
__device__ __forceinline__ void layer_gemm(const QueryParams& p, const LayerDims& d, int l, int w, const float* act,
                                           float* wl, f32x16 (&acc)[kQTiles][2])
{
    const int h = (threadIdx.x & 63) >> 5;
#pragma unroll
    for (int q = 0; q < kQTiles; q++) {
        const int t = w + kQWaves * q;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int f = t * 32 + acc_row(r, h);
            float bv = 0.f;
            if (t < d.tiles) {
                bv = d.b[f < d.n_out ? f : d.n_out - 1];
                bv = f < d.n_out ? bv : 0.f;
            }
            acc[q][0][r] = bv;
            acc[q][1][r] = bv;
        }
    }
    // the wave's tiles w, w + 8: the whole chunk loop is specialised on their number, so the
    // accumulators keep their registers across the chunks
    switch (d.tiles > w ? (d.tiles - w + kQWaves - 1) / kQWaves : 0) {
    case 1: chunk_loop<1>(p, d, l, w, act, wl, acc); break;
    case 2: chunk_loop<2>(p, d, l, w, act, wl, acc); break;
    default: chunk_loop<0>(p, d, l, w, act, wl, acc); break;  // a narrow layer: staging and barriers only
    }
}

__global__ __launch_bounds__(kQThreads) void k_query(const QueryParams p)
{
    extern __shared__ float s_q[];
    float* act = s_q;
    float* wl = s_q + p.act_floats;
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the tile tests are scalar branches
    const int64_t px0 = (int64_t)blockIdx.x * kQPix;

    {  // the pixels' 3 features as rows 0..2 of the activations, row 3 zero; pixels past N zero
        const int f = tid >> 6, px = tid & 63;
        float x = 0.f;
        if (f < 3 && px0 + px < p.N) x = p.feature[(int64_t)f * p.channel_stride + (px0 + px) * p.pixel_stride];
        if (f < 4) act[f * 64 + (px ^ ((f & 1) << 5))] = x;
    }

    f32x16 acc[kQTiles][2];
    for (int l = 0; l + 1 < p.n_layers; l++) {
        const LayerDims d = layer_dims(p, l);
        layer_gemm(p, d, l, w, act, wl, acc);
        // every wave has read its inputs: the outputs replace them, through the next layer's ReLU
#pragma unroll
        for (int q = 0; q < kQTiles; q++) {
            const int t = w + kQWaves * q;
            if (t < d.tiles) {
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int f = t * 32 + acc_row(r, h);
                    if (f < d.n_out) {
                        float* row = act + f * 64;
                        const int sw = (f & 1) << 5;
                        row[j ^ sw] = fmaxf(acc[q][0][r], 0.f);
                        row[(32 + j) ^ sw] = fmaxf(acc[q][1][r], 0.f);
                    }
                }
            }
        }
    }

    // last layer: tiles consumed from the registers
    const LayerDims d = layer_dims(p, p.n_layers - 1);
    const int D = d.n_out, K = p.n_pos + p.n_neg;
    layer_gemm(p, d, p.n_layers - 1, w, act, wl, acc);
    f32x16 dots[2][2];
    float nrm[2] = {0.f, 0.f};
#pragma unroll
    for (int pt = 0; pt < 2; pt++)
#pragma unroll
        for (int r = 0; r < 16; r++) dots[pt][0][r] = dots[pt][1][r] = 0.f;
    // the phrase rows this lane supplies as the A operand (rows past K repeat the last one; their
    // results are never read)
    const float* prow0 = p.phrases + (size_t)(j < K ? j : K - 1) * D;
    const float* prow1 = p.phrases + (size_t)(32 + j < K ? 32 + j : K - 1) * D;
#pragma unroll
    for (int q = 0; q < kQTiles; q++) {
        const int t = w + kQWaves * q;
        if (t < d.tiles) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                nrm[0] = fmaf(acc[q][0][r], acc[q][0][r], nrm[0]);
                nrm[1] = fmaf(acc[q][1][r], acc[q][1][r], nrm[1]);
            }
            if (p.out_decoded) {
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int f = t * 32 + acc_row(r, h);
                    if (f < D) {
                        if (px0 + j < p.N) p.out_decoded[(px0 + j) * D + f] = acc[q][0][r];
                        if (px0 + 32 + j < p.N) p.out_decoded[(px0 + 32 + j) * D + f] = acc[q][1][r];
                    }
                }
            }
            // k step r of the phrase product contracts feature acc_row(r, h) of the tile: registers
            // 4 g .. 4 g + 3 are 4 consecutive features, one float4 of the phrase row
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int f = t * 32 + 8 * g + 4 * h;
                float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
                if (f < D) {
                    a0 = *reinterpret_cast<const float4*>(prow0 + f);
                    if (K > 32) a1 = *reinterpret_cast<const float4*>(prow1 + f);
                }
                const float a0v[4] = {a0.x, a0.y, a0.z, a0.w}, a1v[4] = {a1.x, a1.y, a1.z, a1.w};
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int r = 4 * g + e;
                    dots[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0v[e], acc[q][0][r], dots[0][0], 0, 0, 0);
                    dots[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0v[e], acc[q][1][r], dots[0][1], 0, 0, 0);
                    if (K > 32) {
                        dots[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1v[e], acc[q][0][r], dots[1][0], 0, 0, 0);
                        dots[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1v[e], acc[q][1][r], dots[1][1], 0, 0, 0);
                    }
                }
            }
        }
    }

    // epilogue (layer_gemm's last barrier freed the LDS): red[wave][phrase][px], rn[wave, half][px],
    // nrmf[px], sims[phrase][px]
    const int kpad = K > 32 ? 64 : 32;
    float* red = s_q;
    float* rn = s_q + kQWaves * kpad * 64;
    float* nrmf = rn + 2 * kQWaves * 64;
    float* sims = nrmf + 64;  // [phrase][px]
#pragma unroll
    for (int pt = 0; pt < 2; pt++) {
        if (pt * 32 < kpad) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                float* o = red + (w * kpad + pt * 32 + acc_row(r, h)) * 64 + j;
                o[0] = dots[pt][0][r];
                o[32] = dots[pt][1][r];
            }
        }
    }
    rn[(2 * w + h) * 64 + j] = nrm[0];
    rn[(2 * w + h) * 64 + 32 + j] = nrm[1];
    __syncthreads();
    const int px = tid & 63, grp = tid >> 6;
    float n2 = rn[px];
#pragma unroll
    for (int i = 1; i < 2 * kQWaves; i++) n2 += rn[i * 64 + px];
    const float nv = sqrtf(n2);
    // the K normalised similarities once, into LDS: group g sums phrases g, g + 8, ...
    for (int k = grp; k < K; k += kQWaves) {
        const float* o = red + k * 64 + px;
        float dsum = o[0];
#pragma unroll
        for (int i = 1; i < kQWaves; i++) dsum += o[i * kpad * 64];
        sims[k * 64 + px] = dsum / nv;
    }
    __syncthreads();
    float smax = sims[p.n_pos * 64 + px];
    for (int n = p.n_pos + 1; n < K; n++) smax = fmaxf(smax, sims[n * 64 + px]);
    const bool live = px0 + px < p.N;
    for (int jp = grp; jp < p.n_pos; jp += kQWaves) {
        const float r = 1.0f / (1.0f + expf(10.0f * (smax - sims[jp * 64 + px])));
        if (live) p.out_relevancy[(int64_t)jp * p.N + px0 + px] = r;
    }
    if (p.out_decoded) {  // the stored rows divided by their norms (small N: tests, debugging)
        if (grp == 0) nrmf[px] = nv;
        __threadfence_block();
        __syncthreads();
        for (int idx = tid; idx < 64 * D; idx += kQThreads) {
            const int q = idx / D, f = idx - q * D;
            if (px0 + q < p.N) {
                float* o = p.out_decoded + (px0 + q) * D + f;
                *o = *o / nrmf[q];
            }
        }
    }
}

// lsr_query_semantic: OpenCLIPNetwork.get_semantic_map (eval/openclip_encoder.py:82-94) on the same
// on-chip similarities.  Everything up to and including the sims table is k_query's body without
// out_decoded, over the same __device__ functions; it is a kernel of its own because k_query sits at
// 256 VGPRs with spills and any restructuring of its text (a template over the epilogue, a shared
// body function) changes its code.  Only the epilogue after the second barrier differs:
//     label[px] = first index of the largest s_k (a scan from k = 0 with a strict >: torch.argmax's tie
//                 rule; softmax is monotone, so this is argmax_k softmax(10 s)_k), -1 from n_pos on;
//     score[px] = 1 / sum_k exp(10 (s_k - s_max)), summed in index order: the winner's softmax value.
// All-NaN similarities (a decoded norm of 0) keep index 0 and give a NaN score, as torch.argmax does.
__global__ __launch_bounds__(kQThreads) void k_query_semantic(const QueryParams p, int32_t* out_label, float* out_score)
{
    extern __shared__ float s_q[];
    float* act = s_q;
    float* wl = s_q + p.act_floats;
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t px0 = (int64_t)blockIdx.x * kQPix;

    {
        const int f = tid >> 6, px = tid & 63;
        float x = 0.f;
        if (f < 3 && px0 + px < p.N) x = p.feature[(int64_t)f * p.channel_stride + (px0 + px) * p.pixel_stride];
        if (f < 4) act[f * 64 + (px ^ ((f & 1) << 5))] = x;
    }

    f32x16 acc[kQTiles][2];
    for (int l = 0; l + 1 < p.n_layers; l++) {
        const LayerDims d = layer_dims(p, l);
        layer_gemm(p, d, l, w, act, wl, acc);
#pragma unroll
        for (int q = 0; q < kQTiles; q++) {
            const int t = w + kQWaves * q;
            if (t < d.tiles) {
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int f = t * 32 + acc_row(r, h);
                    if (f < d.n_out) {
                        float* row = act + f * 64;
                        const int sw = (f & 1) << 5;
                        row[j ^ sw] = fmaxf(acc[q][0][r], 0.f);
                        row[(32 + j) ^ sw] = fmaxf(acc[q][1][r], 0.f);
                    }
                }
            }
        }
    }

    const LayerDims d = layer_dims(p, p.n_layers - 1);
    const int D = d.n_out, K = p.n_pos + p.n_neg;
    layer_gemm(p, d, p.n_layers - 1, w, act, wl, acc);
    f32x16 dots[2][2];
    float nrm[2] = {0.f, 0.f};
#pragma unroll
    for (int pt = 0; pt < 2; pt++)
#pragma unroll
        for (int r = 0; r < 16; r++) dots[pt][0][r] = dots[pt][1][r] = 0.f;
    const float* prow0 = p.phrases + (size_t)(j < K ? j : K - 1) * D;
    const float* prow1 = p.phrases + (size_t)(32 + j < K ? 32 + j : K - 1) * D;
#pragma unroll
    for (int q = 0; q < kQTiles; q++) {
        const int t = w + kQWaves * q;
        if (t < d.tiles) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                nrm[0] = fmaf(acc[q][0][r], acc[q][0][r], nrm[0]);
                nrm[1] = fmaf(acc[q][1][r], acc[q][1][r], nrm[1]);
            }
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int f = t * 32 + 8 * g + 4 * h;
                float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
                if (f < D) {
                    a0 = *reinterpret_cast<const float4*>(prow0 + f);
                    if (K > 32) a1 = *reinterpret_cast<const float4*>(prow1 + f);
                }
                const float a0v[4] = {a0.x, a0.y, a0.z, a0.w}, a1v[4] = {a1.x, a1.y, a1.z, a1.w};
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int r = 4 * g + e;
                    dots[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0v[e], acc[q][0][r], dots[0][0], 0, 0, 0);
                    dots[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0v[e], acc[q][1][r], dots[0][1], 0, 0, 0);
                    if (K > 32) {
                        dots[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1v[e], acc[q][0][r], dots[1][0], 0, 0, 0);
                        dots[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1v[e], acc[q][1][r], dots[1][1], 0, 0, 0);
                    }
                }
            }
        }
    }

    // red[wave][phrase][px], rn[wave, half][px], (nrmf unused), sims[phrase][px]: k_query's layout
    const int kpad = K > 32 ? 64 : 32;
    float* red = s_q;
    float* rn = s_q + kQWaves * kpad * 64;
    float* sims = rn + 2 * kQWaves * 64 + 64;
#pragma unroll
    for (int pt = 0; pt < 2; pt++) {
        if (pt * 32 < kpad) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                float* o = red + (w * kpad + pt * 32 + acc_row(r, h)) * 64 + j;
                o[0] = dots[pt][0][r];
                o[32] = dots[pt][1][r];
            }
        }
    }
    rn[(2 * w + h) * 64 + j] = nrm[0];
    rn[(2 * w + h) * 64 + 32 + j] = nrm[1];
    __syncthreads();
    const int px = tid & 63, grp = tid >> 6;
    float n2 = rn[px];
#pragma unroll
    for (int i = 1; i < 2 * kQWaves; i++) n2 += rn[i * 64 + px];
    const float nv = sqrtf(n2);
    for (int k = grp; k < K; k += kQWaves) {
        const float* o = red + k * 64 + px;
        float dsum = o[0];
#pragma unroll
        for (int i = 1; i < kQWaves; i++) dsum += o[i * kpad * 64];
        sims[k * 64 + px] = dsum / nv;
    }
    __syncthreads();
    // one thread group scans: K <= 64 LDS reads per pixel, nothing beside the tile's MFMAs
    if (grp != 0) return;
    float best = sims[px];
    int bi = 0;
    for (int k = 1; k < K; k++) {
        const float v = sims[k * 64 + px];
        if (v > best) {
            best = v;
            bi = k;
        }
    }
    const bool live = px0 + px < p.N;
    if (live) out_label[px0 + px] = bi < p.n_pos ? bi : -1;
    if (out_score) {
        float sum = 0.f;
        for (int k = 0; k < K; k++) sum += expf(10.0f * (sims[k * 64 + px] - best));
        if (live) out_score[px0 + px] = 1.0f / sum;
    }
}

}  // namespace

static size_t query_lds_bytes(QueryParams& p)
{
    int act_rows = 4, max_pad = 0;
    for (int l = 0; l < p.n_layers; l++) {
        if (l + 1 < p.n_layers && p.widths[l] > act_rows) act_rows = p.widths[l];
        const int pad = (p.widths[l] + 31) / 32 * 32;
        if (pad > max_pad) max_pad = pad;
    }
    p.act_floats = act_rows * 64;
    p.ws = max_pad % 64 == 0 ? max_pad + 32 : max_pad;  // 32 mod 64: the A read's lane halves on different banks
    const int kpad = p.n_pos + p.n_neg > 32 ? 64 : 32;
    // red, rn, nrmf, sims: either kernel's epilogue (the semantic scan adds nothing to it)
    const size_t epilogue = 4 * (size_t)(kQWaves * kpad * 64 + 2 * kQWaves * 64 + 64 + kpad * 64);
    for (int kc = 16; kc >= 4; kc >>= 1) {
        const size_t body = 4 * ((size_t)p.act_floats + 2 * (size_t)kc * p.ws);
        if (body <= 160 * 1024 - 1024) {
            p.kc = kc;
            return body > epilogue ? body : epilogue;
        }
    }
    return 0;
}

hipError_t launch_query(QueryParams& p, hipStream_t s, int32_t* out_label, float* out_score)
{
    if (p.N == 0) return hipSuccess;
    const int sem = out_label ? 1 : 0;  // k_query_semantic
    const size_t lds = query_lds_bytes(p);
    if (lds == 0) return hipErrorInvalidValue;
    if (lds > 65536) {
        // dynamic LDS beyond the 64 KiB default is opted into once per device and size: no runtime
        // call on a later launch's path (none inside a stream capture after a warm-up call); each of
        // the two kernels has its own attribute
        static std::mutex mu;
        static size_t allowed[2][64] = {};
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> lock(mu);
        if (dev < 0 || dev >= 64 || allowed[sem][dev] < lds) {
            e = hipFuncSetAttribute(sem ? (const void*)k_query_semantic : (const void*)k_query,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            if (dev >= 0 && dev < 64) allowed[sem][dev] = lds;
        }
    }
    const int64_t blocks = (p.N + kQPix - 1) / kQPix;
    if (sem) hipLaunchKernelGGL(k_query_semantic, dim3((unsigned)blocks), dim3(kQThreads), lds, s, p, out_label, out_score);
    else hipLaunchKernelGGL(k_query, dim3((unsigned)blocks), dim3(kQThreads), lds, s, p);
    return hipGetLastError();
}

}  // namespace lsr
