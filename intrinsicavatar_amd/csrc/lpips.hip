// lpips.hip -- the perceptual distance of systems/criterions.py:105-126 on the device: the VGG-16 trunk of lpips.LPIPS(net="vgg") in f32,
// NHWC (channel innermost: the K dimension of the implicit GEMM is contiguous), and the feature distance of its five taps.
//
//   input stage     [N,H,W,3] in [0,1] -> crop to the rectangle, 2x - 1 on request, the scaling layer (x - shift) / scale -> [N,H,W,4]
//                   (channel 3 = 0) with the crop moved to the buffer's origin
//   conv3x3         pad 1, stride 1, + bias + ReLU as an implicit GEMM on the f32-input MFMA (v_mfma_f32_32x32x2_f32): the result is a
//                   k-ordered fmaf chain in exact f32, the same chain for every pixel whatever tile it falls into
//   maxpool2        2 x 2, stride 2, floor
//   layer distance  per pixel: both feature vectors / (sqrt(sum_c x_c^2) + 1e-10), squared difference x lin[c], summed over c
//   finish          spatial mean per layer and the sum over the five layers, fp64, fixed order -> fp32 value per image + status
//
// THE RECTANGLE IS READ ON THE DEVICE: every kernel takes an optional pointer to (x, y, w, h) int32 (ia_metric_mask_rect's output) and
// works on the extent h >> level, w >> level of it; buffers and grids are sized for the full frame by the host and workgroups outside
// the extent exit.  Whatever lies outside the extent of a buffer is never read (the halo of a convolution is zero there), so a call
// with a rectangle gives the bits of a call on the physically cropped images.  No floating-point atomics: a block of the distance
// kernel owns PPB consecutive pixels OF THE EXTENT, so the partials and their order depend on the rectangle's size alone.
#include <math.h>

#include "ia_common.h"

namespace {

constexpr int TB = 256;                  // threads per block of every kernel here
constexpr int TILE = 16;                 // a workgroup of the convolution owns TILE x TILE pixels x CO output channels
constexpr int HALO = TILE + 2;
constexpr int CK = 16;                   // input channels staged per step
constexpr int CO = 64;
constexpr int IN_STRIDE = CK + 4;        // floats per staged pixel: 16-byte aligned rows, spread over the LDS banks
constexpr int PPB = 64;                  // pixels per partial of the layer distance
constexpr int LAYERS = 5;
constexpr int STATUS_RECT = 2;           // (metrics.hip's: the rectangle does not lie inside the image)
constexpr int STATUS_SMALL = 3;          // a side of the rectangle < 16: nothing is left at the fifth tap

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Ext {
    int x0, y0, w, h;                    // where the window starts in the buffer, and its extent at this level
    bool ok;
};

// H, W: the dimensions of the buffer the window is read from.  at_rect: the window sits at the rectangle's corner (level 0 only);
// otherwise at the buffer's origin, where the input stage moved it.
__device__ inline Ext extent(const int* __restrict__ rect, int H, int W, int level, int at_rect)
{
    Ext e = {0, 0, W, H, true};
    if (rect) {
        int x = rect[0], y = rect[1], w = rect[2], h = rect[3];
        e.ok = x >= 0 && y >= 0 && w >= 0 && h >= 0;
        e.w = e.ok ? w >> level : 0;
        e.h = e.ok ? h >> level : 0;
        e.x0 = at_rect && e.ok ? x : 0;
        e.y0 = at_rect && e.ok ? y : 0;
        if ((int64_t)e.x0 + e.w > W || (int64_t)e.y0 + e.h > H) e.ok = false;
    }
    return e;
}

// ------------------------------------------------------------------------- input stage
__global__ __launch_bounds__(TB) void input_kernel(int H, int W, const float* __restrict__ img, const int* __restrict__ rect, int normalize,
                                                   float* __restrict__ out)
{
    Ext e = extent(rect, H, W, 0, 1);
    if (!e.ok) return;
    const int ox = blockIdx.x * TB + threadIdx.x, oy = blockIdx.y, n = blockIdx.z;
    if (ox >= e.w || oy >= e.h) return;
    const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
    const float* src = img + (((int64_t)n * H + e.y0 + oy) * W + e.x0 + ox) * 3;
    float4 v;
    float* c = &v.x;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float s = src[k];
        if (normalize) s = 2.f * s - 1.f;
        c[k] = (s - shift[k]) / scale[k];
    }
    v.w = 0.f;
    *(float4*)(out + (((int64_t)n * H + oy) * W + ox) * 4) = v;
}

// ------------------------------------------------------------------------- 3 x 3 convolution + bias + ReLU
// GEMM view: M = pixels, N = output channels, K = 9 taps x Cin.  A wave owns 4 rows of the tile = two 32-pixel M tiles, and both 32-channel
// N tiles: 4 accumulators of v_mfma_f32_32x32x2_f32.  Operand maps: lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31];
// D[row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col = l & 31] in register r.  Within a staged step of CK channels the lane half h takes
// channels 8h .. 8h + 7, so its A operands of one tap are two 16-byte LDS reads; the k order is (step, tap, channel in half, half) for every
// output alike.  Channels past Cin (Cin = 4 in the first layer) are staged as zeros: fma(0, 0, c) = c.
__global__ __launch_bounds__(TB) void conv3x3_kernel(int H, int W, int Cin, int Cout, const float* __restrict__ in, const float* __restrict__ wpk,
                                                     const float* __restrict__ bias, float* __restrict__ out, const int* __restrict__ rect,
                                                     int level, int at_rect, int tiles_x)
{
    __shared__ float sIn[HALO * HALO * IN_STRIDE];               // 25.3 KB
    __shared__ float sW[9 * CK * CO];                            // 36 KB
    Ext e = extent(rect, H, W, level, at_rect);
    if (!e.ok) return;
    const int ty0 = (blockIdx.x / tiles_x) * TILE, tx0 = (blockIdx.x % tiles_x) * TILE;
    if (ty0 >= e.h || tx0 >= e.w) return;
    const int co0 = blockIdx.y * CO, n = blockIdx.z;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i = lane & 31, half = lane >> 5;
    const float* in_n = in + (int64_t)n * H * W * Cin;
    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][nt][r] = 0.f;

    for (int c0 = 0; c0 < Cin; c0 += CK) {
        if (c0) __syncthreads();
        for (int idx = t; idx < HALO * HALO * (CK / 4); idx += TB) {
            int pix = idx >> 2, q = idx & 3;
            int hy = pix / HALO, hx = pix - hy * HALO;
            int gy = ty0 + hy - 1, gx = tx0 + hx - 1, c = c0 + q * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gy >= 0 && gy < e.h && gx >= 0 && gx < e.w && c < Cin)
                v = *(const float4*)(in_n + ((int64_t)(e.y0 + gy) * W + (e.x0 + gx)) * Cin + c);
            *(float4*)&sIn[pix * IN_STRIDE + q * 4] = v;
        }
        for (int idx = t; idx < 9 * CK * (CO / 4); idx += TB) {
            int row = idx >> 4, q = idx & 15;                    // row = tap * CK + channel of the step
            int tap = row / CK, c = c0 + (row - tap * CK);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < Cin) v = *(const float4*)(wpk + ((int64_t)tap * Cin + c) * Cout + co0 + q * 4);
            *(float4*)&sW[row * CO + q * 4] = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - ky * 3;
            float a[2][8];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                int hp = (wave * 4 + m * 2 + (i >> 4) + ky) * HALO + (i & 15) + kx;
                float4 lo = *(const float4*)&sIn[hp * IN_STRIDE + half * 8], hi = *(const float4*)&sIn[hp * IN_STRIDE + half * 8 + 4];
                a[m][0] = lo.x, a[m][1] = lo.y, a[m][2] = lo.z, a[m][3] = lo.w;
                a[m][4] = hi.x, a[m][5] = hi.y, a[m][6] = hi.z, a[m][7] = hi.w;
            }
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                const float* wrow = &sW[(tap * CK + half * 8 + kk) * CO + i];
                float b0 = wrow[0], b1 = wrow[32];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0][kk], b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0][kk], b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1][kk], b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1][kk], b1, acc[1][1], 0, 0, 0);
            }
        }
    }
    float* out_n = out + (int64_t)n * H * W * Cout;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int co = co0 + nt * 32 + i;
        const float b = bias[co];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int row = (r & 3) + 8 * (r >> 2) + 4 * half;
                int gy = ty0 + wave * 4 + m * 2 + (row >> 4), gx = tx0 + (row & 15);
                if (gy < e.h && gx < e.w) out_n[((int64_t)gy * W + gx) * Cout + co] = fmaxf(acc[m][nt][r] + b, 0.f);
            }
        }
    }
}

// ------------------------------------------------------------------------- 2 x 2 max-pool, stride 2, floor
__global__ __launch_bounds__(TB) void maxpool2_kernel(int H, int W, int C, const float* __restrict__ in, float* __restrict__ out,
                                                      const int* __restrict__ rect, int level)
{
    Ext e = extent(rect, H, W, level, 0);
    if (!e.ok) return;
    const int Ho = H >> 1, Wo = W >> 1, ho = e.h >> 1, wo = e.w >> 1, c4n = C >> 2;
    const int n = blockIdx.z, oy = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * TB + threadIdx.x;        // (ox, channel quad) of the FULL output row
    const int ox = (int)(j / c4n), c = (int)(j - (int64_t)ox * c4n) * 4;
    if (oy >= ho || ox >= wo) return;
    const float* p = in + (((int64_t)n * H + 2 * oy) * W + 2 * ox) * C + c;
    float4 a = *(const float4*)p, b = *(const float4*)(p + C), d = *(const float4*)(p + (int64_t)W * C), g = *(const float4*)(p + (int64_t)W * C + C);
    float4 v = make_float4(fmaxf(fmaxf(a.x, b.x), fmaxf(d.x, g.x)), fmaxf(fmaxf(a.y, b.y), fmaxf(d.y, g.y)),
                           fmaxf(fmaxf(a.z, b.z), fmaxf(d.z, g.z)), fmaxf(fmaxf(a.w, b.w), fmaxf(d.w, g.w)));
    *(float4*)(out + (((int64_t)n * Ho + oy) * Wo + ox) * C + c) = v;
}

// ------------------------------------------------------------------------- feature distance of one tap
// all 64 lanes end with the same bits: a butterfly adds the same pairs in every lane (a + b = b + a)
__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(TB) void layer_dist_kernel(int H, int W, int C, const float* __restrict__ f0, const float* __restrict__ f1,
                                                        const float* __restrict__ lin, const int* __restrict__ rect, int level,
                                                        double* __restrict__ partials, int64_t cap)
{
    __shared__ double sh[TB / 64];
    Ext e = extent(rect, H, W, level, 0);
    if (!e.ok) return;
    const int64_t npx = (int64_t)e.h * e.w, p0 = (int64_t)blockIdx.x * PPB;
    if (p0 >= npx) return;
    const int n = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int j = wave; j < PPB && p0 + j < npx; j += TB / 64) {
        int64_t p = p0 + j;
        int y = (int)(p / e.w), x = (int)(p - (int64_t)y * e.w);
        const int64_t base = (((int64_t)n * H + y) * W + x) * C;
        double s0 = 0.0, s1 = 0.0;
        for (int c = lane; c < C; c += 64) {
            double a = (double)f0[base + c], b = (double)f1[base + c];
            s0 += a * a;
            s1 += b * b;
        }
        const double n0 = sqrt(wave_sum(s0)) + 1e-10, n1 = sqrt(wave_sum(s1)) + 1e-10;      // an all-zero vector: 0 / 1e-10 = 0
        double d = 0.0;
        for (int c = lane; c < C; c += 64) {
            double diff = (double)f0[base + c] / n0 - (double)f1[base + c] / n1;
            d += (double)lin[c] * (diff * diff);
        }
        acc += wave_sum(d);
    }
    if (lane == 0) sh[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[(int64_t)n * cap + blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// one workgroup per image: per layer the partials of the extent in a fixed order (thread stride, then the LDS tree), / pixels, summed
__global__ __launch_bounds__(TB) void finish_kernel(int N, int H, int W, const int* __restrict__ rect, const double* __restrict__ partials,
                                                    int64_t cap, float* __restrict__ out)
{
    __shared__ double sh[TB];
    const int n = blockIdx.x, t = threadIdx.x;
    Ext e = extent(rect, H, W, 0, 1);
    int status = !e.ok ? STATUS_RECT : (((e.h >> (LAYERS - 1)) < 1 || (e.w >> (LAYERS - 1)) < 1) ? STATUS_SMALL : 0);
    if (status) {
        if (t == 0) {
            out[n] = NAN;
            if (n == 0) out[N] = (float)status;
        }
        return;
    }
    double total = 0.0;
    for (int l = 0; l < LAYERS; ++l) {
        const int64_t npx = (int64_t)(e.h >> l) * (e.w >> l), nblk = (npx + PPB - 1) / PPB;
        const double* p = partials + ((int64_t)l * N + n) * cap;
        double v = 0.0;
        for (int64_t k = t; k < nblk; k += TB) v += p[k];
        sh[t] = v;
        __syncthreads();
        for (int s = TB / 2; s > 0; s >>= 1) {
            if (t < s) sh[t] += sh[t + s];
            __syncthreads();
        }
        total += sh[0] / (double)npx;
        __syncthreads();
    }
    if (t == 0) {
        out[n] = (float)total;
        if (n == 0) out[N] = 0.f;
    }
}

}  // namespace

IA_EXPORT int ia_lpips_pixels_per_partial(void) { return PPB; }

IA_EXPORT int ia_lpips_input(int64_t N, int H, int W, const float* img, const int32_t* rect, int normalize, float* out, ia_stream_t stream)
{
    IA_REQUIRE(N >= 1 && N <= 65535 && H >= 1 && H <= 65535 && W >= 1, "1 <= N, H <= 65535 and W >= 1");
    IA_REQUIRE(img && out, "null pointer");
    hipLaunchKernelGGL(input_kernel, dim3(ia::cdiv(W, TB), H, (int)N), dim3(TB), 0, (hipStream_t)stream, H, W, img, rect, normalize, out);
    return ia::check_launch("ia_lpips_input");
}

IA_EXPORT int ia_lpips_conv3x3(int64_t N, int H, int W, int Cin, int Cout, const float* in, const float* wpk, const float* bias, float* out,
                               const int32_t* rect, int level, int at_rect, ia_stream_t stream)
{
    IA_REQUIRE(N >= 1 && N <= 65535 && H >= 1 && W >= 1, "1 <= N <= 65535 and H, W >= 1");
    IA_REQUIRE(Cin >= 4 && Cin % 4 == 0 && Cout >= CO && Cout % CO == 0 && Cout / CO <= 65535, "Cin a multiple of 4, Cout a multiple of 64");
    IA_REQUIRE(level >= 0 && level < 31 && (!at_rect || level == 0), "0 <= level, and a window at the rectangle's corner only at level 0");
    IA_REQUIRE(in && wpk && bias && out && in != out, "null pointer, or in == out");
    const int tiles_x = ia::cdiv(W, TILE), tiles_y = ia::cdiv(H, TILE);
    IA_REQUIRE((int64_t)tiles_x * tiles_y <= 0x7fffffff, "image too large");
    hipLaunchKernelGGL(conv3x3_kernel, dim3(tiles_x * tiles_y, Cout / CO, (int)N), dim3(TB), 0, (hipStream_t)stream, H, W, Cin, Cout, in, wpk, bias,
                       out, rect, level, at_rect, tiles_x);
    return ia::check_launch("ia_lpips_conv3x3");
}

IA_EXPORT int ia_lpips_maxpool2(int64_t N, int H, int W, int C, const float* in, float* out, const int32_t* rect, int level, ia_stream_t stream)
{
    IA_REQUIRE(N >= 1 && N <= 65535 && H >= 1 && H <= 2 * 65535 && W >= 1, "1 <= N <= 65535, 1 <= H <= 131070 and W >= 1");
    IA_REQUIRE(C >= 4 && C % 4 == 0 && level >= 0 && level < 31, "C a multiple of 4 and 0 <= level");
    if (H < 2 || W < 2) return IA_OK;
    IA_REQUIRE(in && out, "null pointer");
    hipLaunchKernelGGL(maxpool2_kernel, dim3(ia::cdiv((int64_t)(W >> 1) * (C >> 2), TB), H >> 1, (int)N), dim3(TB), 0, (hipStream_t)stream, H, W, C,
                       in, out, rect, level);
    return ia::check_launch("ia_lpips_maxpool2");
}

IA_EXPORT int ia_lpips_layer_dist(int64_t N, int H, int W, int C, const float* f0, const float* f1, const float* lin, const int32_t* rect,
                                  int level, double* partials, int64_t cap, ia_stream_t stream)
{
    IA_REQUIRE(N >= 1 && N <= 65535 && H >= 1 && W >= 1 && C >= 1, "1 <= N <= 65535 and H, W, C >= 1");
    IA_REQUIRE(level >= 0 && level < 31, "0 <= level");
    IA_REQUIRE(f0 && f1 && lin && partials, "null pointer");
    const int64_t nblk = ((int64_t)H * W + PPB - 1) / PPB;
    IA_REQUIRE(nblk <= cap && nblk <= 0x7fffffff, "partials: fewer than ceil(H W / ia_lpips_pixels_per_partial()) per image");
    hipLaunchKernelGGL(layer_dist_kernel, dim3((int)nblk, (int)N), dim3(TB), 0, (hipStream_t)stream, H, W, C, f0, f1, lin, rect, level, partials, cap);
    return ia::check_launch("ia_lpips_layer_dist");
}

IA_EXPORT int ia_lpips_finish(int64_t N, int H, int W, const int32_t* rect, const double* partials, int64_t cap, float* out, ia_stream_t stream)
{
    IA_REQUIRE(N >= 1 && N <= 65535 && H >= 1 && W >= 1, "1 <= N <= 65535 and H, W >= 1");
    IA_REQUIRE(partials && out && cap >= ((int64_t)H * W + PPB - 1) / PPB, "null pointer, or partials too short");
    hipLaunchKernelGGL(finish_kernel, dim3((int)N), dim3(TB), 0, (hipStream_t)stream, (int)N, H, W, rect, partials, cap, out);
    return ia::check_launch("ia_lpips_finish");
}
