// lsr_rgbloss.hip -- the RGB stage's loss (train.py:100-103 with include_feature=False):
//     loss = (1 - lambda) * mean|x - y| + lambda * (1 - ssim(x, y))
// with utils/loss_utils.py:23-63's SSIM (size_average=True): an 11 x 11 Gaussian window g g^T
// (sigma 1.5), zero padding of 5 with no renormalisation at the borders, C1 = 0.01^2, C2 = 0.03^2,
// each of the B * C image planes on its own.  DESIGN.md §6c.
//
//   k_rgb_loss_forward   a workgroup owns a 32 x 32 tile of one plane: stages the tile + 5-pixel
//                        halo of both images in LDS (zero outside the image), 11 taps along x for
//                        x, y, x^2, y^2, xy over the 42 staged rows, 11 taps along y, then per pixel
//                        the SSIM value, |x - y| and (when a gradient is wanted) the three partial
//                        derivatives dS/dmu1, dS/dE[x^2], dS/dE[xy]; one pair of double partial
//                        sums per workgroup
//   k_rgb_loss_reduce    one block adds the partials in index order: deterministic, no float
//                        atomics, nothing to reset between calls
//   k_rgb_loss_backward  the same tiling over the three maps: the window is symmetric, so the
//                        adjoint of the zero-padded correlation is that correlation
#include "lsr_internal.h"

namespace lsr {

constexpr int kRgbThreads = 256;
constexpr int kRgbR = 5;                          // window radius
constexpr int kRgbTaps = 2 * kRgbR + 1;
constexpr int kRgbSH = kRgbTileH + 2 * kRgbR;     // staged rows
constexpr int kRgbSW = kRgbTileW + 2 * kRgbR;     // staged columns
// the row pass puts consecutive rows on consecutive lanes: odd row strides spread the 32 lanes of
// a ds_read_b32 / ds_write_b32 group over the 32 banks
constexpr int kRgbSStride = kRgbSW + 1;           // 43
constexpr int kRgbHStride = kRgbTileW + 1;        // 33
constexpr int kRgbSPlane = kRgbSH * kRgbSStride;  // floats of one staged plane
constexpr int kRgbHPlane = kRgbSH * kRgbHStride;  // floats of one row-pass plane
constexpr int kRgbStageN = kRgbSH * kRgbSW;       // staged samples per plane
constexpr int kRgbStageK = (kRgbStageN + kRgbThreads - 1) / kRgbThreads;  // per thread
constexpr int kRgbPix = kRgbTileH * kRgbTileW / kRgbThreads;              // outputs per thread
constexpr int kRgbRowItems = kRgbSH * (kRgbTileW / 4);  // (row, 4-column group) work items
constexpr int kRgbReduceThreads = 1024;  // ~6 partial pairs per thread at 1080p x 3 planes
static_assert(kRgbTileW == 32 && kRgbTileH % kRgbPix == 0 && kRgbTileW % 4 == 0, "thread mapping of the passes");
static_assert(kRgbThreads / kRgbTileW * kRgbPix == kRgbTileH, "the column pass covers the tile");

// exp(-d^2 / (2 * 1.5^2)) / sum for d = -5 .. 5, normalised in fp64 and rounded to fp32
__device__ constexpr float kRgbG[kRgbTaps] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f,
                                              0x1.b43c40p-3f,  0x1.106560p-2f, 0x1.b43c40p-3f, 0x1.bff0fep-4f,
                                              0x1.26eb18p-5f,  0x1.f1fe02p-8f, 0x1.0d956cp-10f};

struct RgbTile {
    int x0, y0;      // first pixel of the tile
    int64_t base;    // offset of the tile's plane
};

__device__ __forceinline__ RgbTile rgb_tile(int H, int W)
{
    const int tx = (W + kRgbTileW - 1) / kRgbTileW, ty = (H + kRgbTileH - 1) / kRgbTileH;
    const int b = (int)blockIdx.x;
    RgbTile t;
    t.x0 = (b % tx) * kRgbTileW;
    t.y0 = ((b / tx) % ty) * kRgbTileH;
    t.base = (int64_t)(b / (tx * ty)) * ((int64_t)H * W);
    return t;
}

// The tile + halo of kN planes (plane n at src[n], all with the tile's plane offset) into
// st[n][kRgbSH][kRgbSStride], zero outside the image.  Every load of a thread is issued before its
// first LDS store (addresses clamped into the image, the value replaced afterwards).
template <int kN>
__device__ __forceinline__ void rgb_stage(const float* const (&src)[kN], const RgbTile& t, int H, int W, float* st)
{
    float v[kN][kRgbStageK];
#pragma unroll
    for (int k = 0; k < kRgbStageK; k++) {
        const int i = (int)threadIdx.x + k * kRgbThreads;
        const int r = i / kRgbSW, c = i - r * kRgbSW;
        const int gy = t.y0 - kRgbR + r, gx = t.x0 - kRgbR + c;
        const bool in = i < kRgbStageN && gy >= 0 && gy < H && gx >= 0 && gx < W;
        const int cy = min(max(gy, 0), H - 1), cx = min(max(gx, 0), W - 1);
        const int64_t o = t.base + (int64_t)cy * W + cx;
#pragma unroll
        for (int n = 0; n < kN; n++) {
            const float q = src[n][o];
            v[n][k] = in ? q : 0.0f;
        }
    }
#pragma unroll
    for (int k = 0; k < kRgbStageK; k++) {
        const int i = (int)threadIdx.x + k * kRgbThreads;
        const int r = i / kRgbSW, c = i - r * kRgbSW;
        if (i < kRgbStageN) {
#pragma unroll
            for (int n = 0; n < kN; n++) st[n * kRgbSPlane + r * kRgbSStride + c] = v[n][k];
        }
    }
}

// 4 adjacent outputs of the 11-tap filter over 14 consecutive samples, each its own fixed-order sum
__device__ __forceinline__ void rgb_taps4(const float (&q)[kRgbTaps + 3], float (&o)[4])
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float s = kRgbG[0] * q[k];
#pragma unroll
        for (int j = 1; j < kRgbTaps; j++) s = fmaf(kRgbG[j], q[k + j], s);
        o[k] = s;
    }
}

// column pass: outputs (row0 + k, col), k < 4, of one row-pass plane
__device__ __forceinline__ void rgb_cols4(const float* hp, int row0, int col, float (&o)[4])
{
    float q[kRgbTaps + 3];
#pragma unroll
    for (int j = 0; j < kRgbTaps + 3; j++) q[j] = hp[(row0 + j) * kRgbHStride + col];
    rgb_taps4(q, o);
}

// row pass of the forward: quantities kQ0 .. kQ0 + kQN - 1 of {x, y, x^2, y^2, xy} into hs planes
// 0 .. kQN - 1; item = (staged row, group of 4 output columns)
template <int kQ0, int kQN>
__device__ __forceinline__ void rgb_rows_fwd(const float* st, float* hs)
{
    for (int it = (int)threadIdx.x; it < kRgbRowItems; it += kRgbThreads) {
        const int row = it % kRgbSH, c0 = (it / kRgbSH) * 4;
        float x[kRgbTaps + 3], y[kRgbTaps + 3];
#pragma unroll
        for (int j = 0; j < kRgbTaps + 3; j++) {
            x[j] = st[row * kRgbSStride + c0 + j];
            y[j] = st[kRgbSPlane + row * kRgbSStride + c0 + j];
        }
        float* h = hs + row * kRgbHStride + c0;
#pragma unroll
        for (int q = kQ0; q < kQ0 + kQN; q++) {
            float p[kRgbTaps + 3], o[4];
#pragma unroll
            for (int j = 0; j < kRgbTaps + 3; j++)
                p[j] = q == 0 ? x[j] : q == 1 ? y[j] : q == 2 ? x[j] * x[j] : q == 3 ? y[j] * y[j] : x[j] * y[j];
            rgb_taps4(p, o);
#pragma unroll
            for (int k = 0; k < 4; k++) h[(q - kQ0) * kRgbHPlane + k] = o[k];
        }
    }
}

// The five windowed means go through three row-pass planes in two rounds (x, y, x^2, then y^2, xy):
// 31 KB of LDS instead of 42, five workgroups per CU instead of three.
__global__ __launch_bounds__(kRgbThreads, 5) void k_rgb_loss_forward(int H, int W, const float* __restrict__ image,
                                                                     const float* __restrict__ target,
                                                                     float* __restrict__ out_maps,
                                                                     float* __restrict__ out_ssim_map,
                                                                     int64_t map_stride, double* __restrict__ partial)
{
    __shared__ float st[2 * kRgbSPlane];
    __shared__ float hs[3 * kRgbHPlane];
    __shared__ float wsum[2][kRgbThreads / 64];
    const RgbTile t = rgb_tile(H, W);
    const float* const src[2] = {image, target};
    rgb_stage<2>(src, t, H, W, st);
    __syncthreads();

    // column pass: thread = (column, group of kRgbPix output rows)
    const int col = (int)threadIdx.x % kRgbTileW, row0 = ((int)threadIdx.x / kRgbTileW) * kRgbPix;
    float mu1[4], mu2[4], e11[4], e22[4], e12[4];
    rgb_rows_fwd<0, 3>(st, hs);
    __syncthreads();
    rgb_cols4(hs, row0, col, mu1);
    rgb_cols4(hs + kRgbHPlane, row0, col, mu2);
    rgb_cols4(hs + 2 * kRgbHPlane, row0, col, e11);
    __syncthreads();
    rgb_rows_fwd<3, 2>(st, hs);
    __syncthreads();
    rgb_cols4(hs, row0, col, e22);
    rgb_cols4(hs + kRgbHPlane, row0, col, e12);

    const float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);
    float sum_s = 0.0f, sum_l = 0.0f;
    const int gx = t.x0 + col;
#pragma unroll
    for (int k = 0; k < kRgbPix; k++) {
        const int gy = t.y0 + row0 + k;
        if (gy >= H || gx >= W) continue;
        // the reference's operation order (utils/loss_utils.py:47-58)
        const float mu1_sq = mu1[k] * mu1[k], mu2_sq = mu2[k] * mu2[k], mu12 = mu1[k] * mu2[k];
        const float s1 = e11[k] - mu1_sq, s2 = e22[k] - mu2_sq, s12 = e12[k] - mu12;
        const float A = 2.0f * mu12 + C1, B = 2.0f * s12 + C2;
        const float D = mu1_sq + mu2_sq + C1, E = s1 + s2 + C2;
        const float DE = D * E;
        const float S = (A * B) / DE;
        const float xc = st[(row0 + k + kRgbR) * kRgbSStride + col + kRgbR];
        const float yc = st[kRgbSPlane + (row0 + k + kRgbR) * kRgbSStride + col + kRgbR];
        sum_s += S;
        sum_l += fabsf(xc - yc);
        const int64_t o = t.base + (int64_t)gy * W + gx;
        if (out_ssim_map) out_ssim_map[o] = S;
        if (out_maps) {
            // e11 = E[x^2] and e12 = E[xy] as variables of their own beside mu1:
            //   dS/dmu1 = 2 mu2 (B - A) / (DE) + 2 mu1 S (1/E - 1/D),  1/E - 1/D = (D - E) / (DE)
            //   dS/de11 = -S / E = -S D / (DE),  dS/de12 = 2 A / (DE)
            const float r = 1.0f / DE;
            out_maps[o] = (2.0f * mu2[k]) * (B - A) * r + (2.0f * mu1[k]) * S * (D - E) * r;
            out_maps[map_stride + o] = -(S * D) * r;
            out_maps[2 * map_stride + o] = (2.0f * A) * r;
        }
    }

    // workgroup partial sums: wave shuffles, then the waves in order, in double
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum_s += __shfl_xor(sum_s, o, 64);
        sum_l += __shfl_xor(sum_l, o, 64);
    }
    if (lane == 0) {
        wsum[0][wave] = sum_s;
        wsum[1][wave] = sum_l;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < kRgbThreads / 64; w++) {
            a += (double)wsum[0][w];
            b += (double)wsum[1][w];
        }
        partial[2 * (int64_t)blockIdx.x] = a;
        partial[2 * (int64_t)blockIdx.x + 1] = b;
    }
}

// {loss, l1, ssim} from the n workgroup partials: thread i adds partials i, i + 1024, ... in order,
// then a fixed tree over the threads
__global__ __launch_bounds__(kRgbReduceThreads) void k_rgb_loss_reduce(int n, const double* __restrict__ partial,
                                                                        double inv_count, float lambda,
                                                                        float* __restrict__ out_terms)
{
    __shared__ double sa[kRgbReduceThreads], sb[kRgbReduceThreads];
    double a = 0.0, b = 0.0;
    for (int i = (int)threadIdx.x; i < n; i += kRgbReduceThreads) {
        a += partial[2 * (int64_t)i];
        b += partial[2 * (int64_t)i + 1];
    }
    sa[threadIdx.x] = a;
    sb[threadIdx.x] = b;
    __syncthreads();
    for (int s = kRgbReduceThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sa[threadIdx.x] += sa[threadIdx.x + s];
            sb[threadIdx.x] += sb[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float ssim = (float)(sa[0] * inv_count), l1 = (float)(sb[0] * inv_count);
        out_terms[0] = (1.0f - lambda) * l1 + lambda * (1.0f - ssim);  // train.py:101
        out_terms[1] = l1;
        out_terms[2] = ssim;
    }
}

// dL/dx = g [ w_l1 sign(x - y) - w_ssim (conv(Ma) + 2 x conv(Mb) + y conv(Mc)) ],  g = *dL_dloss,
// w_l1 = (1 - lambda) / N, w_ssim = lambda / N
__global__ __launch_bounds__(kRgbThreads) void k_rgb_loss_backward(int H, int W, const float* __restrict__ image,
                                                                   const float* __restrict__ target,
                                                                   const float* __restrict__ maps, int64_t map_stride,
                                                                   const float* __restrict__ dL_dloss, float w_l1,
                                                                   float w_ssim, float* __restrict__ out)
{
    __shared__ float st[3 * kRgbSPlane];
    __shared__ float hs[3 * kRgbHPlane];
    const RgbTile t = rgb_tile(H, W);
    const int col = (int)threadIdx.x % kRgbTileW, row0 = ((int)threadIdx.x / kRgbTileW) * kRgbPix;
    const int gx = t.x0 + col;
    // the thread's own pixels of both images, in flight with the staging loads
    float xc[kRgbPix], yc[kRgbPix];
#pragma unroll
    for (int k = 0; k < kRgbPix; k++) {
        const int64_t o = t.base + (int64_t)min(t.y0 + row0 + k, H - 1) * W + min(gx, W - 1);
        xc[k] = image[o];
        yc[k] = target[o];
    }
    const float g = dL_dloss[0];
    const float* const src[3] = {maps, maps + map_stride, maps + 2 * map_stride};
    rgb_stage<3>(src, t, H, W, st);
    __syncthreads();

    for (int it = (int)threadIdx.x; it < kRgbRowItems; it += kRgbThreads) {
        const int row = it % kRgbSH, c0 = (it / kRgbSH) * 4;
#pragma unroll
        for (int n = 0; n < 3; n++) {
            float q[kRgbTaps + 3], o[4];
#pragma unroll
            for (int j = 0; j < kRgbTaps + 3; j++) q[j] = st[n * kRgbSPlane + row * kRgbSStride + c0 + j];
            rgb_taps4(q, o);
#pragma unroll
            for (int k = 0; k < 4; k++) hs[n * kRgbHPlane + row * kRgbHStride + c0 + k] = o[k];
        }
    }
    __syncthreads();

    float ca[4], cb[4], cc[4];
    rgb_cols4(hs, row0, col, ca);
    rgb_cols4(hs + kRgbHPlane, row0, col, cb);
    rgb_cols4(hs + 2 * kRgbHPlane, row0, col, cc);
#pragma unroll
    for (int k = 0; k < kRgbPix; k++) {
        const int gy = t.y0 + row0 + k;
        if (gy >= H || gx >= W) continue;
        const float d = xc[k] - yc[k];
        const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
        const float ds = ca[k] + (2.0f * xc[k]) * cb[k] + yc[k] * cc[k];
        out[t.base + (int64_t)gy * W + gx] = g * (w_l1 * sg - w_ssim * ds);
    }
}

int64_t rgb_loss_blocks(int planes, int H, int W)
{
    const int64_t tx = (W + kRgbTileW - 1) / kRgbTileW, ty = (H + kRgbTileH - 1) / kRgbTileH;
    return tx * ty * (int64_t)planes;
}

size_t rgb_loss_scratch_bytes(int planes, int H, int W) { return 16 * (size_t)rgb_loss_blocks(planes, H, W); }

hipError_t launch_rgb_loss_forward(const lsr_rgb_loss_args& a, hipStream_t s)
{
    const int nb = (int)rgb_loss_blocks(a.planes, a.H, a.W);
    const int64_t count = (int64_t)a.planes * a.H * a.W;
    double* partial = static_cast<double*>(a.scratch);
    hipLaunchKernelGGL(k_rgb_loss_forward, dim3((unsigned)nb), dim3(kRgbThreads), 0, s, a.H, a.W, a.image, a.target,
                       a.out_maps, a.out_ssim_map, count, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rgb_loss_reduce, dim3(1), dim3(kRgbReduceThreads), 0, s, nb, partial, 1.0 / (double)count,
                       a.lambda_dssim, a.out_terms);
    return hipGetLastError();
}

hipError_t launch_rgb_loss_backward(const lsr_rgb_loss_bwd_args& a, hipStream_t s)
{
    const int nb = (int)rgb_loss_blocks(a.planes, a.H, a.W);
    const int64_t count = (int64_t)a.planes * a.H * a.W;
    const float w_l1 = (float)((1.0 - (double)a.lambda_dssim) / (double)count);
    const float w_ssim = (float)((double)a.lambda_dssim / (double)count);
    hipLaunchKernelGGL(k_rgb_loss_backward, dim3((unsigned)nb), dim3(kRgbThreads), 0, s, a.H, a.W, a.image, a.target,
                       a.maps, count, a.dL_dloss, w_l1, w_ssim, a.out_dL_dimage);
    return hipGetLastError();
}

}  // namespace lsr
