// train_loss.hip -- the loss of one training step (IntrinsicAvatarSystem.training_step, systems/intrinsic_avatar.py:160-301) on the
// model's output dict: fifteen weighted means over the rays and over the samples, forward in two launches (partials, final) and
// backward in one, whichever terms are on.
//
// A translation unit of its own: nothing here is shared with another file's code generation.  The reduction helpers
// repeat those of metrics.hip for that reason: a block owns a fixed slice of the rows, a thread a fixed stride of that slice, the
// block's accumulators are combined by a fixed tree in LDS and one final workgroup combines the blocks' partials the same way.  No
// floating-point atomics, so the same inputs give the same bits on every call.  Every summand is formed in fp64 from the fp32 inputs
// (which widen exactly), every accumulator is fp64; the gradients are rounded to fp32 once, when they are stored.
//
// Nothing is kept between calls: the partials are written before they are read, in every call, for every slot.
#include <math.h>

#include "ia_common.h"

namespace {

constexpr int TB = 256;              // threads per block of every kernel here
constexpr int MAX_BLOCKS = 1024;     // partial-sum blocks over the rays, and as many again over the samples
constexpr int KR = 14;               // doubles of a ray block's partial
constexpr int KS = 3;                // doubles of a sample block's partial
constexpr int K_MAX = KR;

// slots of a ray block's partial
enum { R_RGB_MSE, R_RGB_L1, R_PHYS_MSE, R_PHYS_L1, R_DEMOD, R_MASK_MSE, R_MASK_BCE, R_OPAQUE, R_MAP0, R_MAP1, R_MAP2, R_MAP3, R_NV, R_NVP };
// slots of a sample block's partial
enum { S_EIK, S_SPARSITY, S_CURV };
// term order of terms[] / weights[] (include/ia_amd.h)
enum { T_RGB_MSE, T_RGB_L1, T_PHYS_MSE, T_PHYS_L1, T_DEMOD, T_EIK, T_MASK_MSE, T_MASK_BCE, T_OPAQUE, T_SPARSITY, T_CURV, T_MAP0, T_MAP1,
       T_MAP2, T_MAP3, T_UNUSED };
constexpr int N_TERMS = IA_TRAIN_LOSS_TERMS;
constexpr int ST_NV = N_TERMS, ST_NVP = N_TERMS + 1;      // stats[]: the sixteen terms in fp64, then the two counts

constexpr double OP_LO = 1.0e-3, OP_HI = 1.0 - 1.0e-3;    // torch.clamp(opacity, 1e-3, 1 - 1e-3)

struct Inputs {
    int64_t n, m;
    const float *rgb_full, *phys_full, *demod_full, *opacity;
    const uint8_t *valid, *valid_phys;
    const float *rgb, *rgb_wo_mask, *alpha;
    const float* maps[4];
    const float *sdf, *sdf_grad, *lap;
    float w[N_TERMS];
    float sparsity_scale;
};

struct Grads {
    float *rgb_full, *phys_full, *demod_full, *opacity;
    float* maps[4];
    float *sdf, *sdf_grad, *lap;
};

inline int row_blocks(int64_t n)
{
    int64_t b = (n + TB - 1) / TB;
    return (int)(b > MAX_BLOCKS ? MAX_BLOCKS : b);       // 0 for n == 0
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
__device__ inline void write_partial(double (&v)[K], double* partials, int blk)
{
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) partials[(int64_t)blk * K + k] = v[k];
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

__device__ inline double sgn(double d) { return (double)((d > 0.0) - (d < 0.0)); }

__device__ inline bool in_phys_mask(const Inputs& a, int64_t i) { return a.rgb_wo_mask || !a.valid_phys || a.valid_phys[i]; }

// blocks [0, nrb) own the rays, blocks [nrb, nrb + nsb) the samples
__global__ __launch_bounds__(TB) void train_loss_partial_kernel(Inputs a, int nrb, int nsb, double* __restrict__ partials)
{
    __shared__ double sh[K_MAX * TB];
    const int blk = blockIdx.x;
    if (blk < nrb) {
        const int64_t chunk = (a.n + nrb - 1) / nrb;
        const int64_t b = (int64_t)blk * chunk, e = b + chunk < a.n ? b + chunk : a.n;
        double v[KR];
#pragma unroll
        for (int k = 0; k < KR; ++k) v[k] = 0.0;
        const float* phys_target = a.rgb_wo_mask ? a.rgb_wo_mask : a.rgb;
        for (int64_t i = b + threadIdx.x; i < e; i += TB) {
            const bool val = !a.valid || a.valid[i];
            const bool vp = !a.valid_phys || a.valid_phys[i];
            v[R_NV] += val ? 1.0 : 0.0;
            v[R_NVP] += vp ? 1.0 : 0.0;
            if (a.rgb_full && a.rgb && val) {
                for (int c = 0; c < 3; ++c) {
                    double d = (double)a.rgb_full[i * 3 + c] - (double)a.rgb[i * 3 + c];
                    v[R_RGB_MSE] += d * d;
                    v[R_RGB_L1] += fabs(d);
                }
            }
            if (a.phys_full && phys_target && in_phys_mask(a, i)) {
                for (int c = 0; c < 3; ++c) {
                    double d = (double)a.phys_full[i * 3 + c] - (double)phys_target[i * 3 + c];
                    v[R_PHYS_MSE] += d * d;
                    v[R_PHYS_L1] += fabs(d);
                }
            }
            if (a.demod_full && a.rgb && vp) {
                double l = ((double)a.demod_full[i * 3] + (double)a.demod_full[i * 3 + 1] + (double)a.demod_full[i * 3 + 2]) / 3.0;
                double mx = fmax(fmax((double)a.rgb[i * 3], (double)a.rgb[i * 3 + 1]), (double)a.rgb[i * 3 + 2]);
                v[R_DEMOD] += fabs(l - mx);
            }
            if (a.opacity) {
                double x = fmin(fmax((double)a.opacity[i], OP_LO), OP_HI);
                double lx = log(x), l1x = log(1.0 - x);
                v[R_OPAQUE] -= x * lx + (1.0 - x) * l1x;
                if (a.alpha) {
                    double y = (double)a.alpha[i];
                    v[R_MASK_MSE] += (x - y) * (x - y);
                    v[R_MASK_BCE] -= y * lx + (1.0 - y) * l1x;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (a.maps[k]) v[R_MAP0 + k] += (double)a.maps[k][i];
        }
        block_sum<KR>(v, sh);
        write_partial<KR>(v, partials, blk);
    } else {
        const int sb = blk - nrb;
        const int64_t chunk = (a.m + nsb - 1) / nsb;
        const int64_t b = (int64_t)sb * chunk, e = b + chunk < a.m ? b + chunk : a.m;
        double v[KS] = {0.0, 0.0, 0.0};
        const double scale = (double)a.sparsity_scale;
        for (int64_t j = b + threadIdx.x; j < e; j += TB) {
            if (a.sdf_grad) {
                double gx = a.sdf_grad[j * 3], gy = a.sdf_grad[j * 3 + 1], gz = a.sdf_grad[j * 3 + 2];
                double d = sqrt(gx * gx + gy * gy + gz * gz) - 1.0;
                v[S_EIK] += d * d;
            }
            if (a.sdf) v[S_SPARSITY] += exp(-scale * fabs((double)a.sdf[j]));
            if (a.lap) v[S_CURV] += fabs((double)a.lap[j]);
        }
        block_sum<KS>(v, sh);
        write_partial<KS>(v, partials + (int64_t)nrb * KR, sb);
    }
}

__global__ __launch_bounds__(TB) void train_loss_final_kernel(Inputs a, int nrb, int nsb, const double* __restrict__ partials,
                                                              float* __restrict__ terms, float* __restrict__ loss, double* __restrict__ stats)
{
    __shared__ double sh[K_MAX * TB];
    double r[KR], s[KS];
    final_sum<KR>(partials, nrb, r, sh);
    final_sum<KS>(partials + (int64_t)nrb * KR, nsb, s, sh);
    if (threadIdx.x != 0) return;
    const double n = (double)a.n, m = (double)a.m;
    const double n_phys = a.rgb_wo_mask ? n : r[R_NVP];
    double t[N_TERMS];
    bool on[N_TERMS];
    for (int k = 0; k < N_TERMS; ++k) { t[k] = 0.0; on[k] = false; }
    // a mean over nothing is 0 / 0 = NaN, as torch's
    if (a.rgb_full && a.rgb) {
        t[T_RGB_MSE] = r[R_RGB_MSE] / (3.0 * r[R_NV]);
        t[T_RGB_L1] = r[R_RGB_L1] / (3.0 * r[R_NV]);
        on[T_RGB_MSE] = on[T_RGB_L1] = true;
    }
    if (a.phys_full && (a.rgb_wo_mask || a.rgb)) {
        t[T_PHYS_MSE] = r[R_PHYS_MSE] / (3.0 * n_phys);
        t[T_PHYS_L1] = r[R_PHYS_L1] / (3.0 * n_phys);
        on[T_PHYS_MSE] = on[T_PHYS_L1] = true;
    }
    if (a.demod_full && a.rgb) { t[T_DEMOD] = r[R_DEMOD] / r[R_NVP]; on[T_DEMOD] = true; }
    if (a.sdf_grad) { t[T_EIK] = s[S_EIK] / m; on[T_EIK] = true; }
    if (a.opacity) {
        t[T_OPAQUE] = r[R_OPAQUE] / n;
        on[T_OPAQUE] = true;
        if (a.alpha) {
            t[T_MASK_MSE] = r[R_MASK_MSE] / n;
            t[T_MASK_BCE] = r[R_MASK_BCE] / n;
            on[T_MASK_MSE] = on[T_MASK_BCE] = true;
        }
    }
    if (a.sdf) { t[T_SPARSITY] = s[S_SPARSITY] / m; on[T_SPARSITY] = true; }
    if (a.lap) { t[T_CURV] = s[S_CURV] / m; on[T_CURV] = true; }
    for (int k = 0; k < 4; ++k)
        if (a.maps[k]) { t[T_MAP0 + k] = r[R_MAP0 + k] / n; on[T_MAP0 + k] = true; }
    double total = 0.0;
    for (int k = 0; k < N_TERMS; ++k) {
        if (on[k] && a.w[k] != 0.f) total += (double)a.w[k] * t[k];
        terms[k] = (float)t[k];
        stats[k] = t[k];
    }
    stats[ST_NV] = r[R_NV];
    stats[ST_NVP] = r[R_NVP];
    loss[0] = (float)total;
}

// one thread per ray (blocks [0, nrb)) or per sample (the blocks after them); every given gradient gets every element written
__global__ __launch_bounds__(TB) void train_loss_bwd_kernel(Inputs a, Grads g, int nrb, const double* __restrict__ stats,
                                                            const float* __restrict__ g_loss)
{
    const double gl = (double)g_loss[0];
    if ((int)blockIdx.x < nrb) {
        const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
        if (i >= a.n) return;
        const double n = (double)a.n, nv = stats[ST_NV], nvp = stats[ST_NVP];
        if (g.rgb_full) {
            const bool val = !a.valid || a.valid[i];
            for (int c = 0; c < 3; ++c) {
                double o = 0.0;
                if (val) {
                    double d = (double)a.rgb_full[i * 3 + c] - (double)a.rgb[i * 3 + c];
                    o = gl * ((double)a.w[T_RGB_MSE] * 2.0 * d + (double)a.w[T_RGB_L1] * sgn(d)) / (3.0 * nv);
                }
                g.rgb_full[i * 3 + c] = (float)o;
            }
        }
        if (g.phys_full) {
            const float* target = a.rgb_wo_mask ? a.rgb_wo_mask : a.rgb;
            const bool in = in_phys_mask(a, i);
            const double cnt = a.rgb_wo_mask ? n : nvp;
            for (int c = 0; c < 3; ++c) {
                double o = 0.0;
                if (in) {
                    double d = (double)a.phys_full[i * 3 + c] - (double)target[i * 3 + c];
                    o = gl * ((double)a.w[T_PHYS_MSE] * 2.0 * d + (double)a.w[T_PHYS_L1] * sgn(d)) / (3.0 * cnt);
                }
                g.phys_full[i * 3 + c] = (float)o;
            }
        }
        if (g.demod_full) {
            double o = 0.0;
            if (!a.valid_phys || a.valid_phys[i]) {
                double l = ((double)a.demod_full[i * 3] + (double)a.demod_full[i * 3 + 1] + (double)a.demod_full[i * 3 + 2]) / 3.0;
                double mx = fmax(fmax((double)a.rgb[i * 3], (double)a.rgb[i * 3 + 1]), (double)a.rgb[i * 3 + 2]);
                o = gl * (double)a.w[T_DEMOD] * sgn(l - mx) / (3.0 * nvp);
            }
            for (int c = 0; c < 3; ++c) g.demod_full[i * 3 + c] = (float)o;
        }
        if (g.opacity) {
            double raw = (double)a.opacity[i], o = 0.0;
            if (raw >= OP_LO && raw <= OP_HI) {           // torch's clamp passes the gradient on [min, max], bounds included
                double x = raw;
                o = (double)a.w[T_OPAQUE] * (log(1.0 - x) - log(x));
                if (a.alpha) {
                    double y = (double)a.alpha[i];
                    o += (double)a.w[T_MASK_MSE] * 2.0 * (x - y) - (double)a.w[T_MASK_BCE] * (y / x - (1.0 - y) / (1.0 - x));
                }
                o = gl * o / n;
            }
            g.opacity[i] = (float)o;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (g.maps[k]) g.maps[k][i] = (float)(gl * (double)a.w[T_MAP0 + k] / n);
    } else {
        const int64_t j = ((int64_t)blockIdx.x - nrb) * TB + threadIdx.x;
        if (j >= a.m) return;
        const double m = (double)a.m;
        if (g.sdf_grad) {
            double gx = a.sdf_grad[j * 3], gy = a.sdf_grad[j * 3 + 1], gz = a.sdf_grad[j * 3 + 2];
            double nrm = sqrt(gx * gx + gy * gy + gz * gz);
            double f = nrm > 0.0 ? gl * (double)a.w[T_EIK] * 2.0 * (nrm - 1.0) / (nrm * m) : 0.0;      // the norm's gradient at 0 is 0
            g.sdf_grad[j * 3] = (float)(f * gx);
            g.sdf_grad[j * 3 + 1] = (float)(f * gy);
            g.sdf_grad[j * 3 + 2] = (float)(f * gz);
        }
        if (g.sdf) {
            double sc = (double)a.sparsity_scale, v = (double)a.sdf[j];
            g.sdf[j] = (float)(-gl * (double)a.w[T_SPARSITY] * sc * sgn(v) * exp(-sc * fabs(v)) / m);
        }
        if (g.lap) g.lap[j] = (float)(gl * (double)a.w[T_CURV] * sgn((double)a.lap[j]) / m);
    }
}

inline Inputs pack_inputs(int64_t n, int64_t m, const float* rgb_full, const float* phys_full, const float* demod_full, const float* opacity,
                          const uint8_t* valid, const uint8_t* valid_phys, const float* rgb, const float* rgb_wo_mask, const float* alpha,
                          const float* map0, const float* map1, const float* map2, const float* map3, const float* sdf, const float* sdf_grad,
                          const float* lap, const float* weights, float sparsity_scale)
{
    Inputs a;
    a.n = n;
    a.m = m;
    a.rgb_full = rgb_full;
    a.phys_full = phys_full;
    a.demod_full = demod_full;
    a.opacity = opacity;
    a.valid = valid;
    a.valid_phys = valid_phys;
    a.rgb = rgb;
    a.rgb_wo_mask = rgb_wo_mask;
    a.alpha = alpha;
    a.maps[0] = map0;
    a.maps[1] = map1;
    a.maps[2] = map2;
    a.maps[3] = map3;
    a.sdf = sdf;
    a.sdf_grad = sdf_grad;
    a.lap = lap;
    for (int k = 0; k < N_TERMS; ++k) a.w[k] = weights[k];
    a.sparsity_scale = sparsity_scale;
    return a;
}

}  // namespace

IA_EXPORT int64_t ia_train_loss_partials(int64_t n_rays, int64_t n_samples)
{
    if (n_rays < 0 || n_samples < 0) return -1;
    return (int64_t)row_blocks(n_rays) * KR + (int64_t)row_blocks(n_samples) * KS;
}

IA_EXPORT int ia_train_loss(int64_t n_rays, int64_t n_samples, const float* comp_rgb_full, const float* comp_rgb_phys_full,
                            const float* comp_demod_phys_full, const float* opacity, const uint8_t* rays_valid_full,
                            const uint8_t* rays_valid_phys_full, const float* rgb, const float* rgb_wo_mask, const float* alpha,
                            const float* normals_orientation_loss_map, const float* albedo_smoothness_loss_map,
                            const float* roughness_smoothness_loss_map, const float* metallic_smoothness_loss_map, const float* sdf_samples,
                            const float* sdf_grad_samples, const float* sdf_laplace_samples, const float* weights, float sparsity_scale,
                            float* terms, float* loss, double* stats, double* partials, ia_stream_t stream)
{
    IA_REQUIRE(n_rays >= 0 && n_samples >= 0, "n_rays >= 0 and n_samples >= 0");
    IA_REQUIRE(weights && terms && loss && stats, "null pointer");
    const int nrb = row_blocks(n_rays), nsb = row_blocks(n_samples);
    IA_REQUIRE(partials || nrb + nsb == 0, "null work area");
    Inputs a = pack_inputs(n_rays, n_samples, comp_rgb_full, comp_rgb_phys_full, comp_demod_phys_full, opacity, rays_valid_full,
                           rays_valid_phys_full, rgb, rgb_wo_mask, alpha, normals_orientation_loss_map, albedo_smoothness_loss_map,
                           roughness_smoothness_loss_map, metallic_smoothness_loss_map, sdf_samples, sdf_grad_samples, sdf_laplace_samples,
                           weights, sparsity_scale);
    hipStream_t st = (hipStream_t)stream;
    if (nrb + nsb > 0) hipLaunchKernelGGL(train_loss_partial_kernel, dim3(nrb + nsb), dim3(TB), 0, st, a, nrb, nsb, partials);
    hipLaunchKernelGGL(train_loss_final_kernel, dim3(1), dim3(TB), 0, st, a, nrb, nsb, (const double*)partials, terms, loss, stats);
    return ia::check_launch("ia_train_loss");
}

IA_EXPORT int ia_train_loss_bwd(int64_t n_rays, int64_t n_samples, const float* comp_rgb_full, const float* comp_rgb_phys_full,
                                const float* comp_demod_phys_full, const float* opacity, const uint8_t* rays_valid_full,
                                const uint8_t* rays_valid_phys_full, const float* rgb, const float* rgb_wo_mask, const float* alpha,
                                const float* sdf_samples, const float* sdf_grad_samples, const float* sdf_laplace_samples, const float* weights,
                                float sparsity_scale, const double* stats, const float* g_loss, float* g_comp_rgb_full,
                                float* g_comp_rgb_phys_full, float* g_comp_demod_phys_full, float* g_opacity,
                                float* g_normals_orientation_loss_map, float* g_albedo_smoothness_loss_map,
                                float* g_roughness_smoothness_loss_map, float* g_metallic_smoothness_loss_map, float* g_sdf_samples,
                                float* g_sdf_grad_samples, float* g_sdf_laplace_samples, ia_stream_t stream)
{
    IA_REQUIRE(n_rays >= 0 && n_samples >= 0, "n_rays >= 0 and n_samples >= 0");
    IA_REQUIRE(weights && stats && g_loss, "null pointer");
    IA_REQUIRE(!g_comp_rgb_full || (comp_rgb_full && rgb), "g_comp_rgb_full needs comp_rgb_full and rgb");
    IA_REQUIRE(!g_comp_rgb_phys_full || (comp_rgb_phys_full && (rgb_wo_mask || rgb)), "g_comp_rgb_phys_full needs comp_rgb_phys_full and a target");
    IA_REQUIRE(!g_comp_demod_phys_full || (comp_demod_phys_full && rgb), "g_comp_demod_phys_full needs comp_demod_phys_full and rgb");
    IA_REQUIRE(!g_opacity || opacity, "g_opacity needs opacity");
    IA_REQUIRE(!g_sdf_samples || sdf_samples, "g_sdf_samples needs sdf_samples");
    IA_REQUIRE(!g_sdf_grad_samples || sdf_grad_samples, "g_sdf_grad_samples needs sdf_grad_samples");
    IA_REQUIRE(!g_sdf_laplace_samples || sdf_laplace_samples, "g_sdf_laplace_samples needs sdf_laplace_samples");
    Inputs a = pack_inputs(n_rays, n_samples, comp_rgb_full, comp_rgb_phys_full, comp_demod_phys_full, opacity, rays_valid_full,
                           rays_valid_phys_full, rgb, rgb_wo_mask, alpha, nullptr, nullptr, nullptr, nullptr, sdf_samples, sdf_grad_samples,
                           sdf_laplace_samples, weights, sparsity_scale);
    Grads g;
    g.rgb_full = g_comp_rgb_full;
    g.phys_full = g_comp_rgb_phys_full;
    g.demod_full = g_comp_demod_phys_full;
    g.opacity = g_opacity;
    g.maps[0] = g_normals_orientation_loss_map;
    g.maps[1] = g_albedo_smoothness_loss_map;
    g.maps[2] = g_roughness_smoothness_loss_map;
    g.maps[3] = g_metallic_smoothness_loss_map;
    g.sdf = g_sdf_samples;
    g.sdf_grad = g_sdf_grad_samples;
    g.lap = g_sdf_laplace_samples;
    const bool ray_g = g.rgb_full || g.phys_full || g.demod_full || g.opacity || g.maps[0] || g.maps[1] || g.maps[2] || g.maps[3];
    const bool smp_g = g.sdf || g.sdf_grad || g.lap;
    const int64_t nrb = ray_g ? (n_rays + TB - 1) / TB : 0, nsb = smp_g ? (n_samples + TB - 1) / TB : 0;
    IA_REQUIRE(nrb + nsb < ((int64_t)1 << 31), "too many elements for one launch");
    if (nrb + nsb == 0) return IA_OK;
    hipLaunchKernelGGL(train_loss_bwd_kernel, dim3((unsigned)(nrb + nsb)), dim3(TB), 0, (hipStream_t)stream, a, g, (int)nrb, stats, g_loss);
    return ia::check_launch("ia_train_loss_bwd");
}
