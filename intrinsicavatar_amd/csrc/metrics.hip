// metrics.hip -- frame evaluation on the device (systems/criterions.py:43-102, models/utils.py:268-277,
// systems/intrinsic_avatar.py:303-315 and :396-399): squared error / PSNR, albedo alignment, normal angular error, the bounding
// rectangle of a mask and scikit-image 0.18.1's SSIM over a rectangle that is read from device memory.
//
// Every reduction is DETERMINISTIC: a block owns a fixed slice of the rows, a thread a fixed stride of that slice, the block's 256
// accumulators are combined by a fixed tree in LDS, and one final workgroup combines the blocks' partials the same way -- no
// floating-point atomics anywhere, so the same inputs give the same bits on every run and on every stream.  Accumulators are fp64
// (the fp32 inputs widen exactly).  Nothing here synchronises; a failed precondition that only the device can see (empty mask,
// rectangle smaller than the SSIM window) is reported through a status word next to the value (0 = ok) and the value is NaN.
#include <math.h>

#include "ia_common.h"

namespace {

constexpr int TB = 256;              // threads per block of every kernel here
constexpr int MAX_BLOCKS = 1024;     // partials of a row reduction
constexpr int MAX_K = 8;             // doubles per partial

struct Slice {
    int64_t begin, end;
};

__device__ inline Slice block_slice(int64_t n)
{
    int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
    int64_t b = (int64_t)blockIdx.x * chunk;
    int64_t e = b + chunk < n ? b + chunk : n;
    return {b, e};
}

// fixed-order tree over the block's TB accumulators of K sums each; the result is in v[] of every thread
template <int K>
__device__ inline void block_sum(double (&v)[K], double* sh)
{
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) sh[k * TB + t] = v[k];
    __syncthreads();
    for (int s = TB / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < K; ++k) sh[k * TB + t] += sh[k * TB + t + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = sh[k * TB];
    __syncthreads();
}

template <int K>
__device__ inline void write_partial(double (&v)[K], double* partials)
{
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) partials[(int64_t)blockIdx.x * K + k] = v[k];
    }
}

// sum of the nblk partials (K doubles each) by ONE workgroup, fixed order; result in v[] of every thread
template <int K>
__device__ inline void final_sum(const double* partials, int nblk, double (&v)[K], double* sh)
{
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    for (int i = threadIdx.x; i < nblk; i += TB) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += partials[(int64_t)i * K + k];
    }
    block_sum<K>(v, sh);
}

// ------------------------------------------------------------------------- squared error / PSNR
__global__ __launch_bounds__(TB) void sq_err_partial_kernel(int64_t n, int C, const float* __restrict__ a, const float* __restrict__ b,
                                                            const uint8_t* __restrict__ mask, double* __restrict__ partials)
{
    __shared__ double sh[2 * TB];
    Slice s = block_slice(n);
    double v[2] = {0.0, 0.0};
    for (int64_t i = s.begin + threadIdx.x; i < s.end; i += TB) {
        if (mask && !mask[i]) continue;
        for (int c = 0; c < C; ++c) {
            double d = (double)a[i * C + c] - (double)b[i * C + c];
            v[0] += d * d;
        }
        v[1] += (double)C;
    }
    block_sum<2>(v, sh);
    write_partial<2>(v, partials);
}

__global__ __launch_bounds__(TB) void sq_err_final_kernel(const double* __restrict__ partials, int nblk, double* __restrict__ sums,
                                                          float* __restrict__ psnr)
{
    __shared__ double sh[2 * TB];
    double v[2];
    final_sum<2>(partials, nblk, v, sh);
    if (threadIdx.x == 0) {
        sums[0] = v[0];
        sums[1] = v[1];
        if (psnr) {
            bool ok = v[1] > 0.0;
            psnr[0] = ok ? (float)(-10.0 * log10(v[0] / v[1])) : NAN;
            psnr[1] = ok ? 0.f : 1.f;
        }
    }
}

// ------------------------------------------------------------------------- albedo alignment
__global__ __launch_bounds__(TB) void albedo_sums_partial_kernel(int64_t n, const float* __restrict__ gt, const float* __restrict__ pred,
                                                                 const uint8_t* __restrict__ mask, double* __restrict__ partials)
{
    __shared__ double sh[7 * TB];
    Slice s = block_slice(n);
    double v[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = s.begin + threadIdx.x; i < s.end; i += TB) {
        if (mask && !mask[i]) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double x = (double)gt[i * 3 + c], xh = (double)pred[i * 3 + c];
            v[2 * c] += x * xh;
            v[2 * c + 1] += xh * xh;
        }
        v[6] += 1.0;
    }
    block_sum<7>(v, sh);
    write_partial<7>(v, partials);
}

__global__ __launch_bounds__(TB) void albedo_sums_final_kernel(const double* __restrict__ partials, int nblk, double* __restrict__ sums,
                                                               float* __restrict__ ratio)
{
    __shared__ double sh[7 * TB];
    double v[7];
    final_sum<7>(partials, nblk, v, sh);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 6; ++k) sums[k] = v[k];
        if (ratio) {
            bool ok = v[6] > 0.0;
            for (int c = 0; c < 3; ++c) ratio[c] = ok ? (float)(v[2 * c] / v[2 * c + 1]) : NAN;
            ratio[3] = ok ? 0.f : 1.f;
        }
    }
}

__global__ __launch_bounds__(TB) void albedo_apply_kernel(int64_t n, const float* __restrict__ pred, const uint8_t* __restrict__ mask,
                                                          const float* __restrict__ ratio, float* __restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    bool m = mask ? mask[i] != 0 : true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = ratio[c] * pred[i * 3 + c];
        out[i * 3 + c] = m ? fminf(fmaxf(v, 0.f), 1.f) : 0.f;
    }
}

// ------------------------------------------------------------------------- normals
struct V3 {
    float x, y, z;
};

// transform_normals: normals @ w2c[:3,:3]^T (when a rotation is given), then the OpenCV -> OpenGL flip (1, -1, -1)
__device__ inline V3 to_camera(V3 nrm, const float* __restrict__ R)
{
    V3 o = nrm;
    if (R) {
        o.x = nrm.x * R[0] + nrm.y * R[1] + nrm.z * R[2];
        o.y = nrm.x * R[3] + nrm.y * R[4] + nrm.z * R[5];
        o.z = nrm.x * R[6] + nrm.y * R[7] + nrm.z * R[8];
    }
    o.y = -o.y;
    o.z = -o.z;
    return o;
}

__device__ inline float norm3(V3 v) { return sqrtf(v.x * v.x + v.y * v.y + v.z * v.z); }

// F.normalize(v, dim=-1): v / max(|v|, 1e-12)
__device__ inline V3 normalize3(V3 v)
{
    float d = fmaxf(norm3(v), 1e-12f);
    return {v.x / d, v.y / d, v.z / d};
}

__global__ __launch_bounds__(TB) void transform_normals_kernel(int64_t n, const float* __restrict__ normals, const float* __restrict__ R,
                                                               float* __restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    V3 o = to_camera({normals[i * 3], normals[i * 3 + 1], normals[i * 3 + 2]}, R);
    out[i * 3] = o.x;
    out[i * 3 + 1] = o.y;
    out[i * 3 + 2] = o.z;
}

// NormalError.forward per pixel, in the reference's float32 operations; the sums are fp64
__global__ __launch_bounds__(TB) void normal_error_partial_kernel(int64_t n, const float* __restrict__ pred, const float* __restrict__ target,
                                                                  const uint8_t* __restrict__ mask, const float* __restrict__ R, int transform,
                                                                  int normalize, float* __restrict__ cam_out, float* __restrict__ err_map,
                                                                  double* __restrict__ partials)
{
    __shared__ double sh[2 * TB];
    Slice s = block_slice(n);
    double v[2] = {0.0, 0.0};
    for (int64_t i = s.begin + threadIdx.x; i < s.end; i += TB) {
        V3 a = {pred[i * 3], pred[i * 3 + 1], pred[i * 3 + 2]};
        V3 b = {target[i * 3], target[i * 3 + 1], target[i * 3 + 2]};
        if (transform) a = to_camera(a, R);
        if (cam_out) {
            cam_out[i * 3] = a.x;
            cam_out[i * 3 + 1] = a.y;
            cam_out[i * 3 + 2] = a.z;
        }
        if (normalize) {
            a = normalize3(a);
            b = normalize3(b);
        }
        float inner = a.x * b.x + a.y * b.y + a.z * b.z;
        float c = inner / (norm3(a) * norm3(b) + 1e-8f);
        float m = (mask ? mask[i] != 0 : true) ? 1.f : 0.f;
        float angle = acosf(fminf(fmaxf(c, -1.f), 1.f)) * m;
        float deg = angle * (float)(180.0 / M_PI);
        if (err_map) err_map[i] = deg;
        v[0] += (double)deg;
        v[1] += (double)m;
    }
    block_sum<2>(v, sh);
    write_partial<2>(v, partials);
}

__global__ __launch_bounds__(TB) void normal_error_final_kernel(const double* __restrict__ partials, int nblk, double* __restrict__ sums,
                                                                float* __restrict__ result)
{
    __shared__ double sh[2 * TB];
    double v[2];
    final_sum<2>(partials, nblk, v, sh);
    if (threadIdx.x == 0) {
        sums[0] = v[0];
        sums[1] = v[1];
        if (result) {
            bool ok = v[1] > 0.0;
            result[0] = ok ? (float)(v[0] / v[1]) : NAN;
            result[1] = ok ? 0.f : 1.f;
        }
    }
}

// ------------------------------------------------------------------------- bounding rectangle of a mask
// (min / max of integers: any order gives the same result)
__device__ inline void block_minmax(int (&v)[4], int* sh)
{
    const int t = threadIdx.x;
    for (int k = 0; k < 4; ++k) sh[k * TB + t] = v[k];
    __syncthreads();
    for (int s = TB / 2; s > 0; s >>= 1) {
        if (t < s) {
            sh[t] = min(sh[t], sh[t + s]);
            sh[TB + t] = min(sh[TB + t], sh[TB + t + s]);
            sh[2 * TB + t] = max(sh[2 * TB + t], sh[2 * TB + t + s]);
            sh[3 * TB + t] = max(sh[3 * TB + t], sh[3 * TB + t + s]);
        }
        __syncthreads();
    }
    for (int k = 0; k < 4; ++k) v[k] = sh[k * TB];
    __syncthreads();
}

__global__ __launch_bounds__(TB) void mask_rect_partial_kernel(int H, int W, const uint8_t* __restrict__ mask, int* __restrict__ partials)
{
    __shared__ int sh[4 * TB];
    Slice s = block_slice((int64_t)H * W);
    int v[4] = {W, H, -1, -1};                       // min x, min y, max x, max y
    for (int64_t i = s.begin + threadIdx.x; i < s.end; i += TB) {
        if (!mask[i]) continue;
        int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
        v[0] = min(v[0], x);
        v[1] = min(v[1], y);
        v[2] = max(v[2], x);
        v[3] = max(v[3], y);
    }
    block_minmax(v, sh);
    if (threadIdx.x == 0)
        for (int k = 0; k < 4; ++k) partials[blockIdx.x * 4 + k] = v[k];
}

__global__ __launch_bounds__(TB) void mask_rect_final_kernel(int H, int W, const int* __restrict__ partials, int nblk, int* __restrict__ rect)
{
    __shared__ int sh[4 * TB];
    int v[4] = {W, H, -1, -1};
    for (int i = threadIdx.x; i < nblk; i += TB) {
        v[0] = min(v[0], partials[i * 4]);
        v[1] = min(v[1], partials[i * 4 + 1]);
        v[2] = max(v[2], partials[i * 4 + 2]);
        v[3] = max(v[3], partials[i * 4 + 3]);
    }
    block_minmax(v, sh);
    if (threadIdx.x == 0) {
        bool any = v[2] >= 0;
        rect[0] = any ? v[0] : 0;
        rect[1] = any ? v[1] : 0;
        rect[2] = any ? v[2] - v[0] + 1 : 0;
        rect[3] = any ? v[3] - v[1] + 1 : 0;
    }
}

// ------------------------------------------------------------------------- SSIM (scikit-image 0.18.1 defaults)
constexpr int SSIM_WIN = 7, SSIM_PAD = 3;
constexpr int TS = 32;                               // a workgroup owns TS x TS window centres of one channel
constexpr int TIN = TS + 2 * SSIM_PAD;               // 38: the tile + 3-pixel halo

struct Rect {
    int x, y, w, h, status;                          // status 0 ok, 1 a side < 7, 2 not inside the image
};

__device__ inline Rect load_rect(const int* __restrict__ rect, int H, int W)
{
    Rect r = {0, 0, W, H, 0};
    if (rect) {
        r.x = rect[0];
        r.y = rect[1];
        r.w = rect[2];
        r.h = rect[3];
    }
    if (r.x < 0 || r.y < 0 || r.w < 0 || r.h < 0 || (int64_t)r.x + r.w > W || (int64_t)r.y + r.h > H) r.status = 2;
    else if (r.w < SSIM_WIN || r.h < SSIM_WIN) r.status = 1;
    return r;
}

// The tile grid is anchored at the rectangle's corner and the partial of logical tile (ty, tx) is stored at ty * ntx + tx with ntx taken
// from the RECTANGLE: a masked call and a call on the pre-cropped images add the same numbers in the same order.
__global__ __launch_bounds__(TB) void ssim_tile_kernel(int H, int W, int C, const float* __restrict__ a, const float* __restrict__ b,
                                                       const int* __restrict__ rect, int tile_cap, double* __restrict__ partials)
{
    __shared__ float sa[TIN][TIN], sb[TIN][TIN];                 // 2 x 5.6 KB
    __shared__ double rows[5][TIN][TS];                          // 47.5 KB: 7-tap row sums of x, y, xx, yy, xy
    Rect r = load_rect(rect, H, W);
    if (r.status) return;
    const int ow = r.w - 2 * SSIM_PAD, oh = r.h - 2 * SSIM_PAD;  // window centres that lie wholly inside the rectangle
    const int ntx = (ow + TS - 1) / TS, nty = (oh + TS - 1) / TS;
    const int tx0 = blockIdx.x, ty0 = blockIdx.y, c = blockIdx.z;
    if (tx0 >= ntx || ty0 >= nty) return;
    const int t = threadIdx.x;
    for (int i = t; i < TIN * TIN; i += TB) {
        int iy = i / TIN, ix = i - iy * TIN;
        int ly = ty0 * TS + iy, lx = tx0 * TS + ix;              // inside the rectangle
        float va = 0.f, vb = 0.f;
        if (ly < r.h && lx < r.w) {
            int64_t p = ((int64_t)(r.y + ly) * W + (r.x + lx)) * C + c;
            va = a[p];
            vb = b[p];
        }
        sa[iy][ix] = va;
        sb[iy][ix] = vb;
    }
    __syncthreads();
    for (int i = t; i < TIN * TS; i += TB) {
        int iy = i / TS, col = i - iy * TS;
        double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int j = 0; j < SSIM_WIN; ++j) {
            double x = (double)sa[iy][col + j], y = (double)sb[iy][col + j];
            sx += x;
            sy += y;
            sxx += x * x;
            syy += y * y;
            sxy += x * y;
        }
        rows[0][iy][col] = sx;
        rows[1][iy][col] = sy;
        rows[2][iy][col] = sxx;
        rows[3][iy][col] = syy;
        rows[4][iy][col] = sxy;
    }
    __syncthreads();
    const double inv_np = 1.0 / (SSIM_WIN * SSIM_WIN), cov_norm = (double)(SSIM_WIN * SSIM_WIN) / (SSIM_WIN * SSIM_WIN - 1);
    const double C1 = (0.01 * 2.0) * (0.01 * 2.0), C2 = (0.03 * 2.0) * (0.03 * 2.0);      // (K data_range)^2, data_range = 2
    const int col = t & (TS - 1), r0 = t / TS;
    double acc[1] = {0.0};
    for (int k = 0; k < TS / (TB / TS); ++k) {
        int orow = r0 + k * (TB / TS);
        if (ty0 * TS + orow >= oh || tx0 * TS + col >= ow) continue;
        double m[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double s = 0;
#pragma unroll
            for (int j = 0; j < SSIM_WIN; ++j) s += rows[q][orow + j][col];
            m[q] = s * inv_np;
        }
        double ux = m[0], uy = m[1];
        double vx = cov_norm * (m[2] - ux * ux), vy = cov_norm * (m[3] - uy * uy), vxy = cov_norm * (m[4] - ux * uy);
        double A1 = 2 * ux * uy + C1, A2 = 2 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
        acc[0] += (A1 * A2) / (B1 * B2);
    }
    __syncthreads();
    block_sum<1>(acc, &rows[0][0][0]);
    if (t == 0) partials[(int64_t)c * tile_cap + ty0 * ntx + tx0] = acc[0];
}

__global__ __launch_bounds__(TB) void ssim_final_kernel(int H, int W, int C, const int* __restrict__ rect, int tile_cap,
                                                        const double* __restrict__ partials, double* __restrict__ out)
{
    __shared__ double sh[TB];
    Rect r = load_rect(rect, H, W);
    if (r.status) {
        if (threadIdx.x == 0) {
            out[0] = NAN;
            out[1] = (double)r.status;
        }
        return;
    }
    const int ow = r.w - 2 * SSIM_PAD, oh = r.h - 2 * SSIM_PAD;
    const int ntiles = ((ow + TS - 1) / TS) * ((oh + TS - 1) / TS);
    double total = 0.0;
    for (int c = 0; c < C; ++c) {
        double v[1] = {0.0};
        for (int i = threadIdx.x; i < ntiles; i += TB) v[0] += partials[(int64_t)c * tile_cap + i];
        block_sum<1>(v, sh);
        total += v[0] / ((double)ow * (double)oh);
    }
    if (threadIdx.x == 0) {
        out[0] = total / (double)C;
        out[1] = 0.0;
    }
}

inline int row_blocks(int64_t n)
{
    int64_t b = (n + 4 * TB - 1) / (4 * TB);         // >= 4 rows per thread before another block is worth its partial
    return (int)(b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b));
}

inline int ssim_tiles(int extent) { return extent > 2 * SSIM_PAD ? (extent - 2 * SSIM_PAD + TS - 1) / TS : 1; }

}  // namespace

IA_EXPORT int64_t ia_metric_tmp_bytes(void) { return (int64_t)MAX_BLOCKS * MAX_K * sizeof(double); }

IA_EXPORT int ia_metric_sq_err(int64_t n, int C, const float* a, const float* b, const uint8_t* mask, void* tmp, double* sums, float* psnr,
                               ia_stream_t stream)
{
    IA_REQUIRE(n >= 0 && C >= 1, "n >= 0 and C >= 1");
    IA_REQUIRE(tmp && sums && (n == 0 || (a && b)), "null pointer");
    hipStream_t st = (hipStream_t)stream;
    int nblk = row_blocks(n);
    hipLaunchKernelGGL(sq_err_partial_kernel, dim3(nblk), dim3(TB), 0, st, n, C, a, b, mask, (double*)tmp);
    hipLaunchKernelGGL(sq_err_final_kernel, dim3(1), dim3(TB), 0, st, (const double*)tmp, nblk, sums, psnr);
    return ia::check_launch("ia_metric_sq_err");
}

IA_EXPORT int ia_metric_albedo_sums(int64_t n, const float* gt, const float* pred, const uint8_t* mask, void* tmp, double* sums, float* ratio,
                                    ia_stream_t stream)
{
    IA_REQUIRE(n >= 0, "n >= 0");
    IA_REQUIRE(tmp && sums && (n == 0 || (gt && pred)), "null pointer");
    hipStream_t st = (hipStream_t)stream;
    int nblk = row_blocks(n);
    hipLaunchKernelGGL(albedo_sums_partial_kernel, dim3(nblk), dim3(TB), 0, st, n, gt, pred, mask, (double*)tmp);
    hipLaunchKernelGGL(albedo_sums_final_kernel, dim3(1), dim3(TB), 0, st, (const double*)tmp, nblk, sums, ratio);
    return ia::check_launch("ia_metric_albedo_sums");
}

IA_EXPORT int ia_metric_albedo_apply(int64_t n, const float* pred, const uint8_t* mask, const float* ratio, float* out, ia_stream_t stream)
{
    IA_REQUIRE(n >= 0, "n >= 0");
    if (n == 0) return IA_OK;
    IA_REQUIRE(pred && ratio && out, "null pointer");
    hipLaunchKernelGGL(albedo_apply_kernel, dim3(ia::cdiv(n, TB)), dim3(TB), 0, (hipStream_t)stream, n, pred, mask, ratio, out);
    return ia::check_launch("ia_metric_albedo_apply");
}

IA_EXPORT int ia_metric_transform_normals(int64_t n, const float* normals, const float* w2c_rot, float* out, ia_stream_t stream)
{
    IA_REQUIRE(n >= 0, "n >= 0");
    if (n == 0) return IA_OK;
    IA_REQUIRE(normals && out, "null pointer");
    hipLaunchKernelGGL(transform_normals_kernel, dim3(ia::cdiv(n, TB)), dim3(TB), 0, (hipStream_t)stream, n, normals, w2c_rot, out);
    return ia::check_launch("ia_metric_transform_normals");
}

IA_EXPORT int ia_metric_normal_error(int64_t n, const float* pred, const float* target, const uint8_t* mask, const float* w2c_rot,
                                     int transform, int normalize, float* cam_out, float* err_map, void* tmp, double* sums, float* result,
                                     ia_stream_t stream)
{
    IA_REQUIRE(n >= 0, "n >= 0");
    IA_REQUIRE(tmp && sums && (n == 0 || (pred && target)), "null pointer");
    IA_REQUIRE(transform || (!w2c_rot && !cam_out), "a rotation / camera-space output needs transform = 1");
    hipStream_t st = (hipStream_t)stream;
    int nblk = row_blocks(n);
    hipLaunchKernelGGL(normal_error_partial_kernel, dim3(nblk), dim3(TB), 0, st, n, pred, target, mask, w2c_rot, transform, normalize, cam_out,
                       err_map, (double*)tmp);
    hipLaunchKernelGGL(normal_error_final_kernel, dim3(1), dim3(TB), 0, st, (const double*)tmp, nblk, sums, result);
    return ia::check_launch("ia_metric_normal_error");
}

IA_EXPORT int ia_metric_mask_rect(int H, int W, const uint8_t* mask, void* tmp, int32_t* rect, ia_stream_t stream)
{
    IA_REQUIRE(H >= 1 && W >= 1, "H >= 1 and W >= 1");
    IA_REQUIRE(mask && tmp && rect, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    int nblk = row_blocks((int64_t)H * W);
    hipLaunchKernelGGL(mask_rect_partial_kernel, dim3(nblk), dim3(TB), 0, st, H, W, mask, (int*)tmp);
    hipLaunchKernelGGL(mask_rect_final_kernel, dim3(1), dim3(TB), 0, st, H, W, (const int*)tmp, nblk, rect);
    return ia::check_launch("ia_metric_mask_rect");
}

IA_EXPORT int64_t ia_metric_ssim_tmp_bytes(int H, int W, int C)
{
    if (H < 1 || W < 1 || C < 1) return 0;
    return (int64_t)C * ssim_tiles(W) * ssim_tiles(H) * sizeof(double);
}

IA_EXPORT int ia_metric_ssim(int H, int W, int C, const float* a, const float* b, const int32_t* rect, void* tmp, double* out,
                             ia_stream_t stream)
{
    IA_REQUIRE(H >= 1 && W >= 1 && C >= 1 && C <= 65535, "H, W >= 1 and 1 <= C <= 65535");
    IA_REQUIRE(a && b && tmp && out, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    int gx = ssim_tiles(W), gy = ssim_tiles(H);
    IA_REQUIRE(gy <= 65535, "image too tall");
    hipLaunchKernelGGL(ssim_tile_kernel, dim3(gx, gy, C), dim3(TB), 0, st, H, W, C, a, b, rect, gx * gy, (double*)tmp);
    hipLaunchKernelGGL(ssim_final_kernel, dim3(1), dim3(TB), 0, st, H, W, C, rect, gx * gy, (const double*)tmp, out);
    return ia::check_launch("ia_metric_ssim");
}
