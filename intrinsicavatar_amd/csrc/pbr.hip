// pbr.hip -- Monte-Carlo surface / volume scattering shading for gfx950: BRDF evaluation, environment
// light lookup and pdf, and the light-importance-sampling estimator, fused into one pass per shading
// sample.  Replaces the torch_pbr call chain of IntrinsicAvatarModel.pbr_light_forward
// (models/intrinsic_avatar.py:755-861): scatterer.eval (:806-815), emitter.eval (:819-823),
// emitter.pdf (:830-833), Li / Lo assembly (:824-859).
//
// lib/torch_pbr is an EMPTY submodule in the reference tree: the BRDF and the environment
// light follow the call-site contracts and standard definitions, restated in
// oracle/pbr_ref.py, which is the parity target ("parity unpinned" against upstream torch_pbr):
//   * MultiLobe BRDF = Lambert diffuse lobe + GGX specular lobe (isotropic, alpha = roughness),
//     Smith separable masking, Schlick Fresnel with F0 = lerp(0.04, albedo, metallic); eval returns
//     (diff [1], spec [3]) INCLUDING the cosine foreshortening term (intrinsic_avatar.py:800-803);
//   * EnvironmentLightTensor: equirectangular HDR `base` [H,W,3]; y-up, u = atan2(x,-z)/2pi + 1/2,
//     v = acos(y)/pi; eval = bilinear (wrap in u, clamp in v); pdf(d) = pmf[texel] * H*W/(2 pi^2 sin theta)
//     with pmf proportional to luminance * sin(theta) (pdf_scale = H*W/(2 pi^2), intrinsic_avatar.py:298-300).
// One lane per shading sample; the env map (1024x2048x3 fp32 = 25 MB) and pmf (8 MB) stay in the
// Infinity Cache; algorithmic traffic ~ 100 B in + 36 B out + 4 texels x 12 B per sample.
#include "ia_common.h"

namespace {

constexpr int THREADS = 256;
constexpr float PI_F = 3.14159265358979323846f;

struct EnvMap {
    const float* base;   // [H,W,3]
    const float* pmf;    // [H,W]
    int H, W;
};

__device__ __forceinline__ void dir_to_uv(const float d[3], float& u, float& v)
{
    u = atan2f(d[0], -d[2]) * (0.5f / PI_F) + 0.5f;
    v = acosf(fminf(fmaxf(d[1], -1.0f), 1.0f)) * (1.0f / PI_F);
}

__device__ __forceinline__ void env_eval(const EnvMap& e, const float d[3], float out[3])
{
    float u, v;
    dir_to_uv(d, u, v);
    const float fx = u * e.W - 0.5f, fy = v * e.H - 0.5f;
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float ax = fx - x0f, ay = fy - y0f;
    int x0 = (int)x0f, y0 = (int)y0f;
    int x1 = x0 + 1, y1 = y0 + 1;
    x0 = ((x0 % e.W) + e.W) % e.W;
    x1 = ((x1 % e.W) + e.W) % e.W;
    y0 = min(max(y0, 0), e.H - 1);
    y1 = min(max(y1, 0), e.H - 1);
    const float w00 = (1 - ax) * (1 - ay), w10 = ax * (1 - ay), w01 = (1 - ax) * ay, w11 = ax * ay;
#pragma unroll
    for (int c = 0; c < 3; c++)
        out[c] = w00 * e.base[((int64_t)y0 * e.W + x0) * 3 + c] + w10 * e.base[((int64_t)y0 * e.W + x1) * 3 + c] +
                 w01 * e.base[((int64_t)y1 * e.W + x0) * 3 + c] + w11 * e.base[((int64_t)y1 * e.W + x1) * 3 + c];
}

__device__ __forceinline__ float env_pdf(const EnvMap& e, const float d[3])
{
    float u, v;
    dir_to_uv(d, u, v);
    const int x = min(max((int)(u * e.W), 0), e.W - 1), y = min(max((int)(v * e.H), 0), e.H - 1);
    const float sin_t = sinf((y + 0.5f) * PI_F / e.H);
    return e.pmf[(int64_t)y * e.W + x] * ((float)e.H * (float)e.W / (2.0f * PI_F * PI_F)) / fmaxf(sin_t, 1e-8f);
}

// MultiLobe eval incl. cosine: diff (scalar), spec[3]
__device__ __forceinline__ void brdf_eval(const float n[3], const float wi[3], const float wo[3], float alpha,
                                          const float albedo[3], float metallic, float& diff, float spec[3])
{
    const float NoL = n[0] * wo[0] + n[1] * wo[1] + n[2] * wo[2];
    const float NoV = n[0] * wi[0] + n[1] * wi[1] + n[2] * wi[2];
    diff = 0.0f;
    spec[0] = spec[1] = spec[2] = 0.0f;
    if (NoL <= 0.0f) return;
    diff = NoL * (1.0f / PI_F);
    if (NoV <= 0.0f) return;
    float h[3] = {wi[0] + wo[0], wi[1] + wo[1], wi[2] + wo[2]};
    const float hl = sqrtf(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]);
    if (hl < 1e-12f) return;
    h[0] /= hl; h[1] /= hl; h[2] /= hl;
    const float NoH = n[0] * h[0] + n[1] * h[1] + n[2] * h[2];
    const float VoH = fmaxf(wi[0] * h[0] + wi[1] * h[1] + wi[2] * h[2], 0.0f);
    const float a2 = alpha * alpha;
    const float dd = NoH * NoH * (a2 - 1.0f) + 1.0f;
    const float D = a2 / (PI_F * dd * dd);
    const float G1l = 2.0f * NoL / (NoL + sqrtf(a2 + (1.0f - a2) * NoL * NoL));
    const float G1v = 2.0f * NoV / (NoV + sqrtf(a2 + (1.0f - a2) * NoV * NoV));
    const float om = 1.0f - VoH;
    const float f5 = om * om * om * om * om;
    const float common = D * G1l * G1v / (4.0f * NoV);       // (D G / (4 NoL NoV)) * NoL
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float F0 = 0.04f * (1.0f - metallic) + albedo[c] * metallic;
        spec[c] = common * (F0 + (1.0f - F0) * f5);
    }
}

// MultiLobe sampling density (solid angle): 1/2 cosine-weighted hemisphere + 1/2 GGX half-vector sampling
__device__ __forceinline__ float brdf_pdf(const float n[3], const float wi[3], const float wo[3], float alpha)
{
    const float NoL = n[0] * wo[0] + n[1] * wo[1] + n[2] * wo[2];
    if (NoL <= 0.0f) return 0.0f;
    float p = 0.5f * NoL * (1.0f / PI_F);
    float h[3] = {wi[0] + wo[0], wi[1] + wo[1], wi[2] + wo[2]};
    const float hl = sqrtf(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]);
    if (hl >= 1e-12f) {
        h[0] /= hl; h[1] /= hl; h[2] /= hl;
        const float NoH = n[0] * h[0] + n[1] * h[1] + n[2] * h[2];
        const float VoH = wi[0] * h[0] + wi[1] * h[1] + wi[2] * h[2];
        if (NoH > 0.0f && VoH > 0.0f) {
            const float a2 = alpha * alpha;
            const float dd = NoH * NoH * (a2 - 1.0f) + 1.0f;
            p += 0.5f * (a2 / (PI_F * dd * dd)) * NoH / (4.0f * VoH);
        }
    }
    return p;
}

// orthonormal frame around n (Frisvad / Duff et al.)
__device__ __forceinline__ void frame(const float n[3], float t[3], float b[3])
{
    const float sg = copysignf(1.0f, n[2]);
    const float a = -1.0f / (sg + n[2]);
    const float c = n[0] * n[1] * a;
    t[0] = 1.0f + sg * n[0] * n[0] * a; t[1] = sg * c; t[2] = -sg * n[0];
    b[0] = c; b[1] = sg + n[1] * n[1] * a; b[2] = -n[1];
}

// scatterer.sample: u = (lobe selector, u1, u2)
__device__ __forceinline__ void brdf_sample(const float n[3], const float wi[3], float alpha, const float u[3], float wo[3])
{
    float t[3], b[3];
    frame(n, t, b);
    const float phi = 2.0f * PI_F * u[2];
    if (u[0] < 0.5f) {                               // cosine-weighted hemisphere
        const float r = sqrtf(u[1]), z = sqrtf(fmaxf(1.0f - u[1], 0.0f));
        const float x = r * cosf(phi), y = r * sinf(phi);
#pragma unroll
        for (int c = 0; c < 3; c++) wo[c] = x * t[c] + y * b[c] + z * n[c];
    } else {                                         // GGX normal distribution: cos^2(theta_h) = (1-u)/(1+(a^2-1)u)
        const float a2 = alpha * alpha;
        const float ct = sqrtf(fmaxf((1.0f - u[1]) / (1.0f + (a2 - 1.0f) * u[1]), 0.0f));
        const float st = sqrtf(fmaxf(1.0f - ct * ct, 0.0f));
        float h[3];
#pragma unroll
        for (int c = 0; c < 3; c++) h[c] = st * cosf(phi) * t[c] + st * sinf(phi) * b[c] + ct * n[c];
        const float VoH = wi[0] * h[0] + wi[1] * h[1] + wi[2] * h[2];
#pragma unroll
        for (int c = 0; c < 3; c++) wo[c] = 2.0f * VoH * h[c] - wi[c];
    }
}

__global__ __launch_bounds__(THREADS) void brdf_sample_kernel(int64_t F, const float* __restrict__ normal,
                                                               const float* __restrict__ view_dirs,
                                                               const float* __restrict__ roughness,
                                                               const float* __restrict__ u, float* __restrict__ wo_out)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= F) return;
    const float n[3] = {normal[i * 3], normal[i * 3 + 1], normal[i * 3 + 2]};
    const float wi[3] = {-view_dirs[i * 3], -view_dirs[i * 3 + 1], -view_dirs[i * 3 + 2]};
    const float uu[3] = {u[i * 3], u[i * 3 + 1], u[i * 3 + 2]};
    float wo[3];
    brdf_sample(n, wi, roughness[i], uu, wo);
    wo_out[i * 3] = wo[0]; wo_out[i * 3 + 1] = wo[1]; wo_out[i * 3 + 2] = wo[2];
}

__global__ __launch_bounds__(THREADS) void brdf_pdf_kernel(int64_t F, const float* __restrict__ normal,
                                                            const float* __restrict__ view_dirs,
                                                            const float* __restrict__ wo, const float* __restrict__ roughness,
                                                            float* __restrict__ pdf)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= F) return;
    const float n[3] = {normal[i * 3], normal[i * 3 + 1], normal[i * 3 + 2]};
    const float wi[3] = {-view_dirs[i * 3], -view_dirs[i * 3 + 1], -view_dirs[i * 3 + 2]};
    const float w[3] = {wo[i * 3], wo[i * 3 + 1], wo[i * 3 + 2]};
    pdf[i] = brdf_pdf(n, wi, w, roughness[i]);
}

// ---- lib.torch_pbr scatterer classes: sample / pdf / eval per lobe set -------------------------------------------------
// lobes: 1 = Lambertian (cosine lobe), 2 = GGX (specular lobe), 3 = MultiLobe (both, 1/2 : 1/2 sampling), 4 = Mirror
// (perfect reflection: sample = reflect(wi, n), pdf = 1 -- a discrete direction --, eval = Schlick Fresnel for wo on the
// reflection direction).  wi points AWAY from the surface (the call sites pass -ray direction, intrinsic_avatar.py:559).
__device__ __forceinline__ void lobes_sample(int lobes, const float n[3], const float wi[3], float alpha, const float u[3], float wo[3])
{
    if (lobes == 4) {
        const float c = n[0] * wi[0] + n[1] * wi[1] + n[2] * wi[2];
#pragma unroll
        for (int k = 0; k < 3; k++) wo[k] = 2.0f * c * n[k] - wi[k];
        return;
    }
    float uu[3] = {u[0], u[1], u[2]};
    if (lobes == 1) uu[0] = 0.0f;          // always the cosine lobe
    if (lobes == 2) uu[0] = 1.0f;          // always the GGX lobe
    brdf_sample(n, wi, alpha, uu, wo);
}

__device__ __forceinline__ float lobes_pdf(int lobes, const float n[3], const float wi[3], const float wo[3], float alpha)
{
    if (lobes == 4) return 1.0f;
    const float NoL = n[0] * wo[0] + n[1] * wo[1] + n[2] * wo[2];
    if (NoL <= 0.0f) return 0.0f;
    const float pd = NoL * (1.0f / PI_F);
    if (lobes == 1) return pd;
    const float both = brdf_pdf(n, wi, wo, alpha);                    // 1/2 pd + 1/2 ps
    return lobes == 3 ? both : 2.0f * (both - 0.5f * pd);
}

__global__ __launch_bounds__(THREADS) void scatterer_sample_kernel(int64_t F, int lobes, const float* __restrict__ normal,
                                                                    const float* __restrict__ wi_in, const float* __restrict__ alpha,
                                                                    const float* __restrict__ u, float* __restrict__ wo_out)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= F) return;
    const float n[3] = {normal[i * 3], normal[i * 3 + 1], normal[i * 3 + 2]};
    const float wi[3] = {wi_in[i * 3], wi_in[i * 3 + 1], wi_in[i * 3 + 2]};
    const float uu[3] = {u[i * 3], u[i * 3 + 1], u[i * 3 + 2]};
    float wo[3];
    lobes_sample(lobes, n, wi, alpha[i], uu, wo);
    wo_out[i * 3] = wo[0]; wo_out[i * 3 + 1] = wo[1]; wo_out[i * 3 + 2] = wo[2];
}

__global__ __launch_bounds__(THREADS) void scatterer_pdf_kernel(int64_t F, int lobes, const float* __restrict__ normal,
                                                                 const float* __restrict__ wi_in, const float* __restrict__ wo_in,
                                                                 const float* __restrict__ alpha, float* __restrict__ pdf)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= F) return;
    const float n[3] = {normal[i * 3], normal[i * 3 + 1], normal[i * 3 + 2]};
    const float wi[3] = {wi_in[i * 3], wi_in[i * 3 + 1], wi_in[i * 3 + 2]};
    const float wo[3] = {wo_in[i * 3], wo_in[i * 3 + 1], wo_in[i * 3 + 2]};
    pdf[i] = lobes_pdf(lobes, n, wi, wo, alpha[i]);
}

__global__ __launch_bounds__(THREADS) void scatterer_eval_kernel(int64_t F, int lobes, const float* __restrict__ normal,
                                                                  const float* __restrict__ wi_in, const float* __restrict__ wo_in,
                                                                  const float* __restrict__ alpha, const float* __restrict__ albedo,
                                                                  const float* __restrict__ metallic, float* __restrict__ diff_out,
                                                                  float* __restrict__ spec_out)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= F) return;
    const float n[3] = {normal[i * 3], normal[i * 3 + 1], normal[i * 3 + 2]};
    const float wi[3] = {wi_in[i * 3], wi_in[i * 3 + 1], wi_in[i * 3 + 2]};
    const float wo[3] = {wo_in[i * 3], wo_in[i * 3 + 1], wo_in[i * 3 + 2]};
    const float alb[3] = {albedo[i * 3], albedo[i * 3 + 1], albedo[i * 3 + 2]};
    float diff = 0.0f, spec[3] = {0, 0, 0};
    if (lobes == 4) {
        const float c = n[0] * wi[0] + n[1] * wi[1] + n[2] * wi[2];
        const float r[3] = {2.0f * c * n[0] - wi[0], 2.0f * c * n[1] - wi[1], 2.0f * c * n[2] - wi[2]};
        const float d2 = (r[0] - wo[0]) * (r[0] - wo[0]) + (r[1] - wo[1]) * (r[1] - wo[1]) + (r[2] - wo[2]) * (r[2] - wo[2]);
        if (c > 0.0f && d2 < 1e-6f) {
            const float om = 1.0f - c, f5 = om * om * om * om * om;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float F0 = 0.04f * (1.0f - metallic[i]) + alb[k] * metallic[i];
                spec[k] = F0 + (1.0f - F0) * f5;
            }
        }
    } else {
        brdf_eval(n, wi, wo, alpha[i], alb, metallic[i], diff, spec);
        if (lobes == 1) spec[0] = spec[1] = spec[2] = 0.0f;
        if (lobes == 2) diff = 0.0f;
    }
    diff_out[i] = diff;
    spec_out[i * 3] = spec[0]; spec_out[i * 3 + 1] = spec[1]; spec_out[i * 3 + 2] = spec[2];
}

// Monte-Carlo estimators (one lane per shading sample).  MODE:
//   0 light          pbr_light_forward         :755-861  weight 1/pdf_light (pdf<=0 -> 1), cosine + tr masks
//   1 uniform_light  pbr_uniform_light_forward :654-753  weight inv_pdf[i] (stratified sphere), cosine + tr masks, vis
//   2 mis            pbr_mis_forward           :547-652  weight 1/(pdf_scatter + pdf_light) (0 if <= 1e-6)
//   3 mats           pbr_mats_forward          :863-948  weight 1/pdf_scatter (pdf<=0 -> 1)
template <int MODE>
__global__ __launch_bounds__(THREADS) void pbr_light_kernel(
    int64_t F, const float* __restrict__ inv_pdf, float* __restrict__ vis, const float* __restrict__ normal, const float* __restrict__ albedo, const float* __restrict__ roughness,
    const float* __restrict__ metallic, const float* __restrict__ view_dirs /* t_dirs: wi = -t_dirs */,
    const float* __restrict__ light_dirs /* SMPL space */, const float* __restrict__ tr /* [F] transmittance */,
    const float* __restrict__ ind_rgb /* [F,3] or NULL */, EnvMap env, const float* __restrict__ Rw /* w2s[:3,:3] */,
    float* __restrict__ Lo, float* __restrict__ Lo_diff, float* __restrict__ Lo_spec)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= F) return;
    const float n[3] = {normal[i * 3], normal[i * 3 + 1], normal[i * 3 + 2]};
    const float wo[3] = {light_dirs[i * 3], light_dirs[i * 3 + 1], light_dirs[i * 3 + 2]};
    float lo[3] = {0, 0, 0}, ld[3] = {0, 0, 0}, ls[3] = {0, 0, 0};
    const float cosv = n[0] * wo[0] + n[1] * wo[1] + n[2] * wo[2];
    const bool masked = (MODE == 0 || MODE == 1) ? !(cosv > 1e-6f) : false;       // cosine_mask (:788, :692)
    float t = tr[i];
    if (MODE <= 1) t = fminf(fmaxf(t, 0.0f), 1.0f);                      // secondary_tr.clamp_(0, 1) only in light / uniform_light
    if (masked) t = 0.0f;
    if (MODE == 1 && vis) { vis[i * 3] = 2.0f * t; vis[i * 3 + 1] = 2.0f * t; vis[i * 3 + 2] = 2.0f * t; }
    if (!masked) {
        const float wi[3] = {-view_dirs[i * 3], -view_dirs[i * 3 + 1], -view_dirs[i * 3 + 2]};
        const float alb[3] = {albedo[i * 3], albedo[i * 3 + 1], albedo[i * 3 + 2]};
        const float met = metallic[i];
        float diff, spec[3];
        brdf_eval(n, wi, wo, roughness[i], alb, met, diff, spec);
        float em[3] = {0, 0, 0};
        float w = 1.0f;
        const bool need_env = (MODE >= 2) || (t > 0.0f);                  // tr_mask only in the light / uniform modes
        float pdf_l = 0.0f;
        if (need_env) {
            // transform_dirs_s2w: normalize(d @ w2s[:3,:3])
            float dw[3];
#pragma unroll
            for (int c = 0; c < 3; c++) dw[c] = wo[0] * Rw[0 * 3 + c] + wo[1] * Rw[1 * 3 + c] + wo[2] * Rw[2 * 3 + c];
            const float l = fmaxf(sqrtf(dw[0] * dw[0] + dw[1] * dw[1] + dw[2] * dw[2]), 1e-6f);
            dw[0] /= l; dw[1] /= l; dw[2] /= l;
            env_eval(env, dw, em);
            if (MODE == 0 || MODE == 2) pdf_l = env_pdf(env, dw);
        }
        if (MODE == 0) { w = (need_env && pdf_l > 0.0f) ? 1.0f / pdf_l : 1.0f; }
        else if (MODE == 1) { w = inv_pdf[i]; }
        else {
            const float pdf_s = brdf_pdf(n, wi, wo, roughness[i]);
            if (MODE == 2) { const float sum = pdf_s + pdf_l; w = sum > 1e-6f ? 1.0f / sum : 0.0f; }
            else { w = pdf_s > 0.0f ? 1.0f / pdf_s : 1.0f; }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float Li = em[c] * t + (ind_rgb ? ind_rgb[i * 3 + c] : 0.0f);
            ld[c] = Li * diff * w;
            ls[c] = Li * spec[c] * w;
            lo[c] = (1.0f - met) * alb[c] * ld[c] + ls[c];          // kd = (1-m) albedo, ks = 1
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) { Lo[i * 3 + c] = lo[c]; Lo_diff[i * 3 + c] = ld[c]; Lo_spec[i * 3 + c] = ls[c]; }
}


// ---------------------------------------------------------------------------------------------------------------
// Backward of the light / uniform_light estimators (training with PBR losses, BASELINE config 4).  The reference gets
// these gradients from autograd through scatterer.eval and emitter.eval (intrinsic_avatar.py:705-745, :806-859);
// directions, transmittance, masks and sampling weights are constants (computed under no_grad there).
//   Lo_c = (kd_c diff + spec_c) Li_c w ,  kd = (1-m) albedo ,  Li = em(dir) tr (+ indirect)
//   spec_c = common (F0_c + (1 - F0_c) f5) ,  common = D G1(NoL) G1(NoV) / (4 NoV) ,  F0 = 0.04 (1-m) + albedo m
// outputs: d/d normal [F,3], albedo [F,3], roughness [F], metallic [F]; d/d env texels accumulated with atomics.
__device__ __forceinline__ void env_footprint(const EnvMap& e, const float d[3], int& x0, int& x1, int& y0, int& y1, float& ax, float& ay)
{
    float u, v;
    dir_to_uv(d, u, v);
    const float fx = u * e.W - 0.5f, fy = v * e.H - 0.5f;
    const float x0f = floorf(fx), y0f = floorf(fy);
    ax = fx - x0f; ay = fy - y0f;
    x0 = (int)x0f; y0 = (int)y0f;
    x1 = x0 + 1; y1 = y0 + 1;
    x0 = ((x0 % e.W) + e.W) % e.W;
    x1 = ((x1 % e.W) + e.W) % e.W;
    y0 = min(max(y0, 0), e.H - 1);
    y1 = min(max(y1, 0), e.H - 1);
}

__device__ __forceinline__ void env_scatter(const EnvMap& e, float* __restrict__ g_base, const float d[3], const float g[3])
{
    int x0, x1, y0, y1;
    float ax, ay;
    env_footprint(e, d, x0, x1, y0, y1, ax, ay);
    const float w00 = (1 - ax) * (1 - ay), w10 = ax * (1 - ay), w01 = (1 - ax) * ay, w11 = ax * ay;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (g[c] == 0.0f) continue;
        unsafeAtomicAdd(g_base + ((int64_t)y0 * e.W + x0) * 3 + c, w00 * g[c]);
        unsafeAtomicAdd(g_base + ((int64_t)y0 * e.W + x1) * 3 + c, w10 * g[c]);
        unsafeAtomicAdd(g_base + ((int64_t)y1 * e.W + x0) * 3 + c, w01 * g[c]);
        unsafeAtomicAdd(g_base + ((int64_t)y1 * e.W + x1) * 3 + c, w11 * g[c]);
    }
}

// d L / d env texels for large batches.  env_scatter above issues 12 device-scope float atomics per visible sample and those
// execute at the memory side of the fabric (~21 G/s wherever they land): 31 ms for the 98.6 M samples of the headline step,
// against 3 ms for everything else the backward kernel does.  Instead the backward kernel leaves one 24-byte record per sample
// (texel x0 | y0 << 16 | (y1 == y0) << 31, the two bilinear fractions, the three channel gradients) and this kernel adds the
// records up in LDS: the map is cut into horizontal bands of TH rows (+1 row for the y1 neighbours: <= 112 KB of LDS), the
// samples into n_ranges contiguous ranges, one workgroup per (range, band) streams the range's records, keeps those whose y0
// lies in its band, and finally adds its band to g_base with one atomic per touched texel channel.  The bands of one range
// run on one XCD (workgroup index modulo 8), so that a range's records come out of that XCD's L2 after the first reader.
constexpr uint32_t ENV_REC_NONE = 0xFFFFFFFFu;
constexpr int ENV_ACC_THREADS = 1024;
constexpr int ENV_ACC_LDS = 112 * 1024;             // band accumulator; + 32 KB of wave queues: 144 of the CU's 160 KB
constexpr int ENV_Q = 512;                           // queue entries per wave (a stretch of 4 records per lane adds <= 256)

__global__ __launch_bounds__(ENV_ACC_THREADS) void env_band_accumulate_kernel(int64_t F, const uint32_t* __restrict__ rec_idx,
                                                                              const float2* __restrict__ rec_w,
                                                                              const float* __restrict__ rec_g, int H, int W, int TH,
                                                                              int n_bands, int n_ranges, float* __restrict__ g_base)
{
    extern __shared__ float s_acc[];                    // [(TH + 1)][W][3]
    const int b = blockIdx.x;
    const int q = b >> 3;
    const int band = q % n_bands, range = (b & 7) + 8 * (q / n_bands);
    if (range >= n_ranges) return;
    const int y_lo = band * TH;
    const int rows = min(TH + 1, H - y_lo);
    for (int e = threadIdx.x; e < rows * W * 3; e += ENV_ACC_THREADS) s_acc[e] = 0.0f;
    __syncthreads();
    const int64_t per = ((F + n_ranges - 1) / n_ranges + 3) & ~(int64_t)3;         // multiple of 4: 16-byte index loads
    const int64_t i0 = (int64_t)range * per, i1 = min(F, i0 + per);
    // Only ~1 record in 2 n_bands belongs to this band: a wave first collects the matching records of a stretch in its own LDS
    // queue (ballot + prefix append, no barrier: a wave's LDS operations execute in order) and then works the queue off with
    // all lanes busy -- 64 records' weight / gradient loads in flight together and full-width LDS atomics.  (Handling a match
    // where it is found costs every wave the whole matched path, two dependent global loads included, for one or two lanes:
    // 9.3 ms per step instead of ~2.)
    __shared__ uint32_t s_q[ENV_ACC_THREADS / 64][ENV_Q];        // offsets from i0 of the queued records
    uint32_t* wq = s_q[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    int nq = 0;                                                    // wave-uniform
    auto drain = [&]() {
        for (int e = lane; e < nq; e += 64) {
            const int64_t i = i0 + wq[e];
            const uint32_t k = rec_idx[i];
            const int y0 = (int)((k >> 16) & 0x7FFFu) - y_lo;
            const int x0 = (int)(k & 0xFFFFu);
            const int x1 = x0 + 1 == W ? 0 : x0 + 1;
            const int y1 = (k >> 31) ? y0 : y0 + 1;
            const float2 a = rec_w[i];
            const float w00 = (1 - a.x) * (1 - a.y), w10 = a.x * (1 - a.y), w01 = (1 - a.x) * a.y, w11 = a.x * a.y;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float g = rec_g[i * 3 + c];
                if (g == 0.0f) continue;
                atomicAdd(&s_acc[(y0 * W + x0) * 3 + c], w00 * g);
                atomicAdd(&s_acc[(y0 * W + x1) * 3 + c], w10 * g);
                atomicAdd(&s_acc[(y1 * W + x0) * 3 + c], w01 * g);
                atomicAdd(&s_acc[(y1 * W + x1) * 3 + c], w11 * g);
            }
        }
        nq = 0;
    };
    auto push = [&](int64_t i, uint32_t k) {
        const int y0 = (int)((k >> 16) & 0x7FFFu) - y_lo;
        const bool m = k != ENV_REC_NONE && y0 >= 0 && y0 < TH;
        const uint64_t bal = __ballot(m);
        if (m) wq[nq + __popcll(bal & ((1ull << lane) - 1ull))] = (uint32_t)(i - i0);
        nq += __popcll(bal);
    };
    // trip counts are wave-uniform (push() ballots): whole strides of 8 records per thread first, then guarded strides of 4
    const bool a16 = (reinterpret_cast<uintptr_t>(rec_idx) & 15) == 0;
    const int64_t n = i1 > i0 ? i1 - i0 : 0;
    const int64_t n8 = a16 ? n / (8 * ENV_ACC_THREADS) : 0;
    int64_t i = i0 + (int64_t)threadIdx.x * 4;
    for (int64_t it = 0; it < n8; it++, i += 8 * ENV_ACC_THREADS) {
        const uint4 k0 = *reinterpret_cast<const uint4*>(rec_idx + i);
        const uint4 k1 = *reinterpret_cast<const uint4*>(rec_idx + i + 4 * ENV_ACC_THREADS);
        push(i, k0.x); push(i + 1, k0.y); push(i + 2, k0.z); push(i + 3, k0.w);
        if (nq > ENV_Q - 4 * 64) drain();
        const int64_t j = i + 4 * ENV_ACC_THREADS;
        push(j, k1.x); push(j + 1, k1.y); push(j + 2, k1.z); push(j + 3, k1.w);
        if (nq > ENV_Q - 4 * 64) drain();
    }
    const int64_t rest0 = i0 + n8 * 8 * ENV_ACC_THREADS;
    const int64_t n4 = (i1 - rest0 + 4 * ENV_ACC_THREADS - 1) / (4 * ENV_ACC_THREADS);
    i = rest0 + (int64_t)threadIdx.x * 4;
    for (int64_t it = 0; it < n4; it++, i += 4 * ENV_ACC_THREADS) {
#pragma unroll
        for (int u = 0; u < 4; u++) push(i + u, i + u < i1 ? rec_idx[i + u] : ENV_REC_NONE);
        if (nq > ENV_Q - 4 * 64) drain();
    }
    drain();
    __syncthreads();
    float* gb = g_base + (int64_t)y_lo * W * 3;
    for (int e = threadIdx.x; e < rows * W * 3; e += ENV_ACC_THREADS) {
        const float v = s_acc[e];
        if (v != 0.0f) unsafeAtomicAdd(gb + e, v);
    }
}

// ---- the same sums from records BINNED BY BAND, in fixed point -----------------------------------------------------------------------
// Two things were wrong with env_band_accumulate_kernel.  (1) It reads the 4-byte texel words of ALL records once per band (16
// bands for the reference's 256 x 512 map) and then gathers the matching records' weights and gradients -- one record in 16, an
// 8- and a 12-byte piece out of every ~380 bytes: PMC 14.8 GB per launch for 2.0 GB of records.  (2) What it spends its time on
// is something else: LDS float atomics.  With the records binned and read contiguously the accumulation alone still took
// 3.66 ms per headline step; the same kernel with INTEGER LDS atomics 0.27 ms, with plain (racy) read-modify-writes 0.36 ms, without
// its flush 3.64 ms -- ds_add_f32 runs at ~0.5 lanes per clock and CU on gfx950, ds_add_u32 / u64 at the LDS's rate.
// So: records are binned by band (count per 8192-record tile + max |g| -> one exclusive scan over [band][tile] -> scatter as
// 24-byte AoS records: all streamed), and a band's list is summed in 64-bit FIXED POINT: contribution = round(w g S), S =
// 2^(62 - ceil(log2 F)) / max |g| (a texel channel receives at most F contributions of at most max |g|: the signed 64-bit sum cannot
// wrap whatever the batch size; the headline's F = 83 M gives 2^35: a contribution keeps its 24 fp32 bits down to 2^-11 of the
// largest one and is absolute to 2^-35 of it below: tighter than any fp32 summation order), LDS ds_add_u64, one global 64-bit
// atomic per touched texel channel into an integer image, converted and added to g_base once per texel at the end.  Integer
// sums do not depend on the order: the texel gradient is bit-reproducible run to run (the float-atomic versions were not).
constexpr int ENV_TILE = 8192;
constexpr int ENV_ACC64_LDS = 144 * 1024;

__global__ __launch_bounds__(ENV_ACC_THREADS) void env_bin_count_kernel(int64_t F, const uint32_t* __restrict__ rec_idx,
                                                                        const float* __restrict__ rec_g, int TH, int n_bands, int n_tiles,
                                                                        int32_t* __restrict__ counts /*[n_bands][n_tiles]*/,
                                                                        uint32_t* __restrict__ gmax /* bits of max |g| */)
{
    __shared__ int s_h[32];
    __shared__ uint32_t s_m;
    if (threadIdx.x < 32) s_h[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_m = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * ENV_TILE;
    float m = 0.0f;
#pragma unroll
    for (int j = 0; j < ENV_TILE / ENV_ACC_THREADS; j++) {
        const int64_t i = base + j * ENV_ACC_THREADS + threadIdx.x;
        const uint32_t k = i < F ? rec_idx[i] : ENV_REC_NONE;
        const int b = k != ENV_REC_NONE ? (int)((k >> 16) & 0x7FFFu) / TH : -1;
        if (b >= 0) m = fmaxf(m, fmaxf(fabsf(rec_g[i * 3]), fmaxf(fabsf(rec_g[i * 3 + 1]), fabsf(rec_g[i * 3 + 2]))));
#pragma unroll 1
        for (int bb = 0; bb < n_bands; bb++) {
            const uint64_t mk = __ballot(b == bb);
            if (mk && (threadIdx.x & 63) == 0) atomicAdd(&s_h[bb], __popcll(mk));
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(&s_m, __float_as_uint(m));       // non-negative floats order like their bits
    __syncthreads();
    if (threadIdx.x < n_bands) counts[(int64_t)threadIdx.x * n_tiles + blockIdx.x] = s_h[threadIdx.x];
    if (threadIdx.x == 0 && s_m > *gmax) atomicMax(gmax, s_m);                           // read first: same-address atomics serialise
}

struct EnvRec { uint32_t k; float ax, ay, g0, g1, g2; };      // 24 bytes

__global__ __launch_bounds__(ENV_ACC_THREADS) void env_bin_scatter_kernel(int64_t F, const uint32_t* __restrict__ rec_idx,
                                                                          const float2* __restrict__ rec_w, const float* __restrict__ rec_g,
                                                                          int TH, int n_bands, int n_tiles, const int32_t* __restrict__ offs,
                                                                          EnvRec* __restrict__ out)
{
    __shared__ int s_cur[32];                                     // next free slot of (this tile, band) in the band-sorted list
    if (threadIdx.x < n_bands) s_cur[threadIdx.x] = offs[(int64_t)threadIdx.x * n_tiles + blockIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * ENV_TILE;
#pragma unroll
    for (int j = 0; j < ENV_TILE / ENV_ACC_THREADS; j++) {
        const int64_t i = base + j * ENV_ACC_THREADS + threadIdx.x;
        const uint32_t k = i < F ? rec_idx[i] : ENV_REC_NONE;
        const int b = k != ENV_REC_NONE ? (int)((k >> 16) & 0x7FFFu) / TH : -1;
        int pos = -1;
#pragma unroll 1
        for (int bb = 0; bb < n_bands; bb++) {
            const uint64_t m = __ballot(b == bb);
            if (!m) continue;
            int wbase = 0;
            if (lane == 0) wbase = atomicAdd(&s_cur[bb], __popcll(m));
            wbase = __builtin_amdgcn_readfirstlane(wbase);
            if (b == bb) pos = wbase + __popcll(m & ((1ull << lane) - 1ull));
        }
        if (pos >= 0) {
            const float2 a = rec_w[i];
            EnvRec r;
            r.k = k; r.ax = a.x; r.ay = a.y; r.g0 = rec_g[i * 3]; r.g1 = rec_g[i * 3 + 1]; r.g2 = rec_g[i * 3 + 2];
            out[pos] = r;
        }
    }
}

// fixed-point scale of the band sums: 2^shift / max |g| with shift = 62 - ceil(log2 F) (host): a texel channel receives at most F
// contributions of at most max |g| each, so the signed 64-bit sum cannot wrap whatever the batch size (F = 83 M: shift 35)
__device__ __forceinline__ double env_fixed_scale(uint32_t gmax_bits, int shift)
{
    const float m = __uint_as_float(gmax_bits);
    return (m > 0.0f && m < 3.0e38f) ? __longlong_as_double((long long)(1023 + shift) << 52) / (double)m : 0.0;
}

__global__ __launch_bounds__(ENV_ACC_THREADS) void env_band_accumulate_binned_kernel(const EnvRec* __restrict__ recs,
                                                                                     const int32_t* __restrict__ offs /*[n_bands][n_tiles]*/,
                                                                                     const int32_t* __restrict__ total_p, int n_tiles, int H, int W,
                                                                                     int TH, int n_bands, const uint32_t* __restrict__ gmax, int shift,
                                                                                     unsigned long long* __restrict__ acc64 /*[H][W][3]*/)
{
    extern __shared__ unsigned long long s_acc64[];     // [(TH + 1)][W][3], two's complement
    // which (band, part) is this workgroup: parts of a band = ceil(records of the band / R), R = records per workgroup
    const int total = *total_p;
    const double S = env_fixed_scale(*gmax, shift);
    if (total == 0 || S == 0.0) return;
    const int R = max(4096, (total + ((int)gridDim.x - n_bands) - 1) / max((int)gridDim.x - n_bands, 1));
    int band = -1, part = 0, b0 = 0, b1 = 0;
    {
        int w = blockIdx.x;
        for (int b = 0; b < n_bands; b++) {
            const int s0 = offs[(int64_t)b * n_tiles], s1 = b + 1 < n_bands ? offs[(int64_t)(b + 1) * n_tiles] : total;
            const int parts = (s1 - s0 + R - 1) / R;
            if (w < parts) { band = b; part = w; b0 = s0; b1 = s1; break; }
            w -= parts;
        }
    }
    if (band < 0) return;
    const int y_lo = band * TH;
    const int rows = min(TH + 1, H - y_lo);
    for (int e = threadIdx.x; e < rows * W * 3; e += ENV_ACC_THREADS) s_acc64[e] = 0ull;
    __syncthreads();
    const int i0 = b0 + part * R, i1 = min(b1, i0 + R);
    for (int i = i0 + threadIdx.x; i < i1; i += ENV_ACC_THREADS) {
        const EnvRec r = recs[i];
        const int y0 = (int)((r.k >> 16) & 0x7FFFu) - y_lo;
        const int x0 = (int)(r.k & 0xFFFFu);
        const int x1 = x0 + 1 == W ? 0 : x0 + 1;
        const int y1 = (r.k >> 31) ? y0 : y0 + 1;
        const float w00 = (1 - r.ax) * (1 - r.ay), w10 = r.ax * (1 - r.ay), w01 = (1 - r.ax) * r.ay, w11 = r.ax * r.ay;
        const float g[3] = {r.g0, r.g1, r.g2};
        auto add = [&](int e, float v) { atomicAdd(&s_acc64[e], (unsigned long long)__double2ll_rn((double)v * S)); };
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if (g[c] == 0.0f) continue;
            add((y0 * W + x0) * 3 + c, w00 * g[c]);          // the fp32 products of the float versions, summed exactly
            add((y0 * W + x1) * 3 + c, w10 * g[c]);
            add((y1 * W + x0) * 3 + c, w01 * g[c]);
            add((y1 * W + x1) * 3 + c, w11 * g[c]);
        }
    }
    __syncthreads();
    unsigned long long* gb = acc64 + (int64_t)y_lo * W * 3;
    for (int e = threadIdx.x; e < rows * W * 3; e += ENV_ACC_THREADS) {
        const unsigned long long v = s_acc64[e];
        if (v != 0ull) atomicAdd(gb + e, v);
    }
}

__global__ __launch_bounds__(THREADS) void env_fixed_finish_kernel(int64_t n, const unsigned long long* __restrict__ acc64,
                                                                    const uint32_t* __restrict__ gmax, int shift, float* __restrict__ g_base)
{
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (e >= n) return;
    const long long v = (long long)acc64[e];
    if (v == 0) return;
    g_base[e] += (float)((double)v / env_fixed_scale(*gmax, shift));
}

template <int MODE>
__global__ __launch_bounds__(THREADS) void pbr_light_bwd_kernel(
    int64_t F, const float* __restrict__ inv_pdf, const float* __restrict__ normal, const float* __restrict__ albedo,
    const float* __restrict__ roughness, const float* __restrict__ metallic, const float* __restrict__ view_dirs,
    const float* __restrict__ light_dirs, const float* __restrict__ tr, const float* __restrict__ ind_rgb, EnvMap env,
    const float* __restrict__ Rw, const float* __restrict__ g_Lo, const float* __restrict__ g_Ld,
    const float* __restrict__ g_Ls, float* __restrict__ g_normal, float* __restrict__ g_albedo,
    float* __restrict__ g_rough, float* __restrict__ g_metal, float* __restrict__ g_base, uint32_t* __restrict__ rec_idx,
    float2* __restrict__ rec_w, float* __restrict__ rec_g)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= F) return;
    if (rec_idx) rec_idx[i] = ENV_REC_NONE;
    float gn[3] = {0, 0, 0}, ga[3] = {0, 0, 0}, gr = 0.0f, gm = 0.0f;
    const float n[3] = {normal[i * 3], normal[i * 3 + 1], normal[i * 3 + 2]};
    const float wo[3] = {light_dirs[i * 3], light_dirs[i * 3 + 1], light_dirs[i * 3 + 2]};
    const float NoL = n[0] * wo[0] + n[1] * wo[1] + n[2] * wo[2];
    if (NoL > 1e-6f) {                                                    // cosine_mask
        const float t = fminf(fmaxf(tr[i], 0.0f), 1.0f);
        const float wi[3] = {-view_dirs[i * 3], -view_dirs[i * 3 + 1], -view_dirs[i * 3 + 2]};
        const float alb[3] = {albedo[i * 3], albedo[i * 3 + 1], albedo[i * 3 + 2]};
        const float met = metallic[i], alpha = roughness[i];
        float em[3] = {0, 0, 0}, dw[3] = {0, 0, 1};
        float w = 1.0f;
        if (t > 0.0f) {
#pragma unroll
            for (int c = 0; c < 3; c++) dw[c] = wo[0] * Rw[0 * 3 + c] + wo[1] * Rw[1 * 3 + c] + wo[2] * Rw[2 * 3 + c];
            const float l = fmaxf(sqrtf(dw[0] * dw[0] + dw[1] * dw[1] + dw[2] * dw[2]), 1e-6f);
            dw[0] /= l; dw[1] /= l; dw[2] /= l;
            env_eval(env, dw, em);
            if (MODE == 0) { const float p = env_pdf(env, dw); w = p > 0.0f ? 1.0f / p : 1.0f; }
        }
        if (MODE == 1) w = inv_pdf[i];
        float diff, spec[3];
        brdf_eval(n, wi, wo, alpha, alb, met, diff, spec);
        // c_c = d L / d (kd diff + spec)_c ; gradients that arrive on Lo_diff / Lo_spec directly are folded in
        float gLi[3], cd[3], cs[3];
        float gdiff = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float Li = em[c] * t + (ind_rgb ? ind_rgb[i * 3 + c] : 0.0f);
            const float glo = g_Lo ? g_Lo[i * 3 + c] : 0.0f;
            const float gld = (g_Ld ? g_Ld[i * 3 + c] : 0.0f) + glo * (1.0f - met) * alb[c];     // on Li diff w
            const float gls = (g_Ls ? g_Ls[i * 3 + c] : 0.0f) + glo;                              // on Li spec w
            cd[c] = gld * Li * w;              // d / d diff   (per channel, summed below)
            cs[c] = gls * Li * w;              // d / d spec_c
            gdiff += cd[c];
            gLi[c] = (gld * diff + gls * spec[c]) * w;
            // kd = (1-m) albedo multiplies Li diff w inside Lo only
            const float ldw = Li * diff * w;
            ga[c] += glo * (1.0f - met) * ldw;
            gm += glo * (-alb[c]) * ldw;
        }
        float gNoL = gdiff * (1.0f / PI_F), gNoV = 0.0f, gNoH = 0.0f;
        const float NoV = n[0] * wi[0] + n[1] * wi[1] + n[2] * wi[2];
        float h[3] = {wi[0] + wo[0], wi[1] + wo[1], wi[2] + wo[2]};
        const float hl = sqrtf(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]);
        if (NoV > 0.0f && hl >= 1e-12f) {
            h[0] /= hl; h[1] /= hl; h[2] /= hl;
            const float NoH = n[0] * h[0] + n[1] * h[1] + n[2] * h[2];
            const float VoH = fmaxf(wi[0] * h[0] + wi[1] * h[1] + wi[2] * h[2], 0.0f);
            const float a2 = alpha * alpha;
            const float dd = NoH * NoH * (a2 - 1.0f) + 1.0f;
            const float D = a2 / (PI_F * dd * dd);
            const float sl = sqrtf(a2 + (1.0f - a2) * NoL * NoL), sv = sqrtf(a2 + (1.0f - a2) * NoV * NoV);
            const float G1l = 2.0f * NoL / (NoL + sl), G1v = 2.0f * NoV / (NoV + sv);
            const float om = 1.0f - VoH;
            const float f5 = om * om * om * om * om;
            const float common = D * G1l * G1v / (4.0f * NoV);
            float gcommon = 0.0f;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float F0 = 0.04f * (1.0f - met) + alb[c] * met;
                const float Fr = F0 + (1.0f - F0) * f5;
                gcommon += cs[c] * Fr;
                const float gF0 = cs[c] * common * (1.0f - f5);
                ga[c] += gF0 * met;
                gm += gF0 * (alb[c] - 0.04f);
            }
            const float k = gcommon / (4.0f * NoV);
            const float gD = k * G1l * G1v, gG1l = k * D * G1v, gG1v = k * D * G1l;
            gNoV += -gcommon * common / NoV;
            float ga2 = gD * (1.0f / (PI_F * dd * dd) - 2.0f * a2 * NoH * NoH / (PI_F * dd * dd * dd));
            gNoH += gD * (-4.0f * a2 * NoH * (a2 - 1.0f) / (PI_F * dd * dd * dd));
            {   // G1(x) = 2x / (x + s), s = sqrt(a2 + (1 - a2) x^2)
                const float dl = (NoL + sl) * (NoL + sl), dv = (NoV + sv) * (NoV + sv);
                gNoL += gG1l * (2.0f * (NoL + sl) - 2.0f * NoL * (1.0f + (1.0f - a2) * NoL / sl)) / dl;
                gNoV += gG1v * (2.0f * (NoV + sv) - 2.0f * NoV * (1.0f + (1.0f - a2) * NoV / sv)) / dv;
                ga2 += gG1l * (-2.0f * NoL / dl) * (1.0f - NoL * NoL) / (2.0f * sl);
                ga2 += gG1v * (-2.0f * NoV / dv) * (1.0f - NoV * NoV) / (2.0f * sv);
            }
            gr = 2.0f * alpha * ga2;
#pragma unroll
            for (int c = 0; c < 3; c++) gn[c] += gNoH * h[c] + gNoV * wi[c];
        }
#pragma unroll
        for (int c = 0; c < 3; c++) gn[c] += gNoL * wo[c];
        if (g_base && t > 0.0f) {
            const float ge[3] = {gLi[0] * t, gLi[1] * t, gLi[2] * t};
            if (rec_idx) {                          // deferred: env_band_accumulate_kernel adds the records up in LDS
                int x0, x1, y0, y1;
                float ax, ay;
                env_footprint(env, dw, x0, x1, y0, y1, ax, ay);
                rec_idx[i] = (uint32_t)x0 | ((uint32_t)y0 << 16) | (y1 == y0 ? 0x80000000u : 0u);
                rec_w[i] = make_float2(ax, ay);
                rec_g[i * 3 + 0] = ge[0]; rec_g[i * 3 + 1] = ge[1]; rec_g[i * 3 + 2] = ge[2];
            } else {
                env_scatter(env, g_base, dw, ge);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) { g_normal[i * 3 + c] = gn[c]; g_albedo[i * 3 + c] = ga[c]; }
    g_rough[i] = gr;
    g_metal[i] = gm;
}

__global__ __launch_bounds__(THREADS) void env_eval_kernel(int64_t n, const float* __restrict__ dirs_world, EnvMap env,
                                                            float* __restrict__ rgb, float* __restrict__ pdf)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const float d[3] = {dirs_world[i * 3], dirs_world[i * 3 + 1], dirs_world[i * 3 + 2]};
    if (rgb) { float o[3]; env_eval(env, d, o); rgb[i * 3] = o[0]; rgb[i * 3 + 1] = o[1]; rgb[i * 3 + 2] = o[2]; }
    if (pdf) pdf[i] = env_pdf(env, d);
}

// ---- add_emitter: the emitter's radiance along camera rays (models/intrinsic_avatar.py:1319-1333, :1455-1490) ---------------------------
// transform_dirs_s2w (snarf_deformer.py:154-158): normalize(d @ w2s[:3,:3]) -- the matrix itself, not its transpose; |x| clamped at 1e-6
__device__ __forceinline__ void dirs_s2w(const float d[3], const float* __restrict__ Rw, float dw[3])
{
    // every operation spelled out (no contraction left to the compiler): the kernels that share this function agree bit for bit
#pragma unroll
    for (int c = 0; c < 3; c++) dw[c] = __fmaf_rn(d[2], Rw[2 * 3 + c], __fmaf_rn(d[1], Rw[1 * 3 + c], __fmul_rn(d[0], Rw[0 * 3 + c])));
    const float l = fmaxf(__fsqrt_rn(__fmaf_rn(dw[2], dw[2], __fmaf_rn(dw[1], dw[1], __fmul_rn(dw[0], dw[0])))), 1e-6f);
    dw[0] = __fdiv_rn(dw[0], l); dw[1] = __fdiv_rn(dw[1], l); dw[2] = __fdiv_rn(dw[2], l);
}

// one lane per ray: 12 B in, 12 B out, 4 texels x 12 B from the cached map.  Either output may be NULL: `dirs_world` alone is
// ia_transform_dirs_s2w -- the same kernel, so the directions it shows are the ones the lookup used
__global__ __launch_bounds__(THREADS) void env_background_kernel(int64_t n, const float* __restrict__ rays_d, const float* __restrict__ Rw,
                                                                  EnvMap env, float* __restrict__ out, float* __restrict__ dirs_world)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const float d[3] = {rays_d[i * 3], rays_d[i * 3 + 1], rays_d[i * 3 + 2]};
    float dw[3];
    dirs_s2w(d, Rw, dw);
    if (dirs_world) { dirs_world[i * 3] = dw[0]; dirs_world[i * 3 + 1] = dw[1]; dirs_world[i * 3 + 2] = dw[2]; }
    if (out) {
        float o[3];
        env_eval(env, dw, o);
        out[i * 3] = o[0]; out[i * 3 + 1] = o[1]; out[i * 3 + 2] = o[2];
    }
}

// backward w.r.t. the texels, in the 64-bit fixed point of the band path above (env_fixed_scale / env_fixed_finish_kernel): max |g| first,
// then every ray adds round(w g S) to the caller's integer image with global 64-bit integer atomics -- integer sums do not depend on the
// order, so the gradient is bit-reproducible.  A frame has ~3 10^5 rays (3.5 M atomics, microseconds at the fabric's ~21 G/s): the record /
// bin / band machinery, built for 10^8 shading samples, would only add launches here.
__global__ __launch_bounds__(THREADS) void env_absmax_kernel(int64_t n3, const float* __restrict__ g, uint32_t* __restrict__ gmax)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    float m = i < n3 ? fabsf(g[i]) : 0.0f;
    if (!(m == m)) m = 3.4e38f;                              // NaN: env_fixed_scale turns the whole gradient off, as for an infinite one
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(gmax, __float_as_uint(m));        // non-negative floats order like their bits
}

__global__ __launch_bounds__(THREADS) void env_background_bwd_kernel(int64_t n, const float* __restrict__ rays_d, const float* __restrict__ Rw,
                                                                      EnvMap env, const float* __restrict__ g_out,
                                                                      const uint32_t* __restrict__ gmax, int shift,
                                                                      unsigned long long* __restrict__ acc64)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const double S = env_fixed_scale(*gmax, shift);
    if (S == 0.0) return;
    const float d[3] = {rays_d[i * 3], rays_d[i * 3 + 1], rays_d[i * 3 + 2]};
    float dw[3];
    dirs_s2w(d, Rw, dw);
    int x0, x1, y0, y1;
    float ax, ay;
    env_footprint(env, dw, x0, x1, y0, y1, ax, ay);          // indices wrapped / clamped into [0, W) x [0, H)
    const float w00 = (1 - ax) * (1 - ay), w10 = ax * (1 - ay), w01 = (1 - ax) * ay, w11 = ax * ay;
    const int W = env.W;
    auto add = [&](int64_t e, float v) { atomicAdd(&acc64[e], (unsigned long long)__double2ll_rn((double)v * S)); };
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float g = g_out[i * 3 + c];
        if (g == 0.0f) continue;
        add(((int64_t)y0 * W + x0) * 3 + c, w00 * g);
        add(((int64_t)y0 * W + x1) * 3 + c, w10 * g);
        add(((int64_t)y1 * W + x0) * 3 + c, w01 * g);
        add(((int64_t)y1 * W + x1) * 3 + c, w11 * g);
    }
}

}  // namespace

IA_EXPORT int ia_pbr_shade(int mode, int64_t F, const float* normal, const float* albedo, const float* roughness,
                           const float* metallic, const float* view_dirs, const float* out_dirs, const float* transmittance,
                           const float* indirect_rgb, const float* inv_pdf, const float* env_base, const float* env_pmf,
                           int env_h, int env_w, const float* w2s_rot, float* Lo, float* Lo_diff, float* Lo_spec,
                           float* vis, ia_stream_t stream)
{
    if (F == 0) return IA_OK;
    IA_REQUIRE(env_h > 0 && env_w > 0, "environment map must be non-empty");
    IA_REQUIRE(mode >= 0 && mode <= 3, "mode: 0 light, 1 uniform_light, 2 mis, 3 mats");
    IA_REQUIRE(mode != 1 || inv_pdf != nullptr, "uniform_light needs inv_pdf");
    EnvMap e{env_base, env_pmf, env_h, env_w};
    const int grid = ia::cdiv(F, THREADS);
    hipStream_t s = (hipStream_t)stream;
#define IA_PBR_LAUNCH(M) pbr_light_kernel<M><<<grid, THREADS, 0, s>>>(F, inv_pdf, vis, normal, albedo, roughness, metallic, \
        view_dirs, out_dirs, transmittance, indirect_rgb, e, w2s_rot, Lo, Lo_diff, Lo_spec)
    if (mode == 0) IA_PBR_LAUNCH(0);
    else if (mode == 1) IA_PBR_LAUNCH(1);
    else if (mode == 2) IA_PBR_LAUNCH(2);
    else IA_PBR_LAUNCH(3);
#undef IA_PBR_LAUNCH
    return ia::check_launch("ia_pbr_shade");
}


// batches below this scatter the image gradient with atomics directly; IA_ENV_ACC_MIN_F overrides (A/B runs).  2^18: the 4096-ray training
// batch at spp 512 has 2.09 M foreground points (just under the former 2^21) and its backward took 1.33 ms with direct atomics on the
// 256 x 512 training light against 0.2 ms through the band-sorted records (config-4 step 15.7 -> 14.3 ms, same box)
static int64_t env_acc_min_f()
{
    static const int64_t v = [] { const char* e = getenv("IA_ENV_ACC_MIN_F"); return e ? (int64_t)atoll(e) : ((int64_t)1 << 18); }();
    return v;
}
#define ENV_ACC_MIN_F env_acc_min_f()
constexpr size_t ENV_FIXED_MAX_TEXELS = (size_t)1 << 21;       // 1024 x 2048
extern "C" int64_t ia_scan_tmp_bytes(int64_t n);
extern "C" int ia_exclusive_scan_i32(const int32_t* in, int32_t* out, int32_t* total, int64_t n, void* tmp, ia_stream_t stream);

// work area of the banded image-gradient path: SoA records of the backward kernel (24 B each) | band-sorted AoS records | [32][n_tiles]
// counts | the same, scanned | total | max |g| | scan work area | the 64-bit fixed-point image (sized for the largest map the fixed-point
// path takes: 2^21 texels).  scratch 16-byte aligned.
struct EnvBwdScratch {
    uint32_t* rec_idx;
    float2* rec_w;
    float* rec_g;
    EnvRec* sorted;
    int32_t *counts, *offs, *total;
    uint32_t* gmax;
    void* scan_tmp;
    unsigned long long* acc64;
    bool fits;
};

static size_t env_bwd_layout(void* scratch, size_t bytes, int64_t F, EnvBwdScratch* o)
{
    const size_t n4 = ((size_t)F + 3) & ~(size_t)3;
    const size_t n_tiles = ((size_t)F + ENV_TILE - 1) / ENV_TILE;
    ia::Carver c(scratch, bytes);
    o->rec_idx = c.take<uint32_t>(n4, 16);            // the three record columns lie back to back (n4 is a multiple of 4)
    o->rec_w = c.take<float2>(n4, 16);
    o->rec_g = c.take<float>(3 * n4, 16);
    c.skip(64);
    o->sorted = c.take<EnvRec>(n4, 16);
    o->counts = c.take<int32_t>(32 * n_tiles, 16);
    c.skip(64);
    o->offs = c.take<int32_t>(32 * n_tiles, 16);
    c.skip(64);
    o->total = c.take<int32_t>(4, 16);
    o->gmax = c.take<uint32_t>(12, 16);
    o->scan_tmp = c.take<char>((size_t)ia_scan_tmp_bytes((int64_t)(32 * n_tiles)));
    o->acc64 = c.take<unsigned long long>(ENV_FIXED_MAX_TEXELS * 3);
    c.skip(256);                                          // tail slack, as the callers have always allocated
    o->fits = c.fits();
    return c.need(16);
}

IA_EXPORT size_t ia_pbr_shade_bwd_scratch_bytes(int64_t F)
{
    if (F < ENV_ACC_MIN_F) return 0;                 // small batches scatter with atomics directly
    EnvBwdScratch w;
    return env_bwd_layout(nullptr, SIZE_MAX, F, &w);
}

IA_EXPORT int ia_pbr_shade_bwd(int mode, int64_t F, const float* normal, const float* albedo, const float* roughness,
                               const float* metallic, const float* view_dirs, const float* out_dirs,
                               const float* transmittance, const float* indirect_rgb, const float* inv_pdf,
                               const float* env_base, const float* env_pmf, int env_h, int env_w, const float* w2s_rot,
                               const float* g_Lo, const float* g_Lo_diff, const float* g_Lo_spec, float* g_normal,
                               float* g_albedo, float* g_roughness, float* g_metallic, float* g_env_base, void* scratch,
                               size_t scratch_bytes, ia_stream_t stream)
{
    if (F == 0) return IA_OK;
    IA_REQUIRE(mode == 0 || mode == 1, "backward is provided for the training estimators: 0 light, 1 uniform_light");
    IA_REQUIRE(mode != 1 || inv_pdf != nullptr, "uniform_light needs inv_pdf");
    IA_REQUIRE(g_normal && g_albedo && g_roughness && g_metallic, "all four per-point gradient outputs are required");
    EnvMap e{env_base, env_pmf, env_h, env_w};
    const int grid = ia::cdiv(F, THREADS);
    hipStream_t s = (hipStream_t)stream;
    // large batches with a caller-provided scratch: records + banded LDS accumulation instead of 12 fabric atomics per sample
    uint32_t* rec_idx = nullptr;
    float2* rec_w = nullptr;
    float* rec_g = nullptr;
    EnvBwdScratch w{};
    int TH = 0, n_bands = 0;
    if (g_env_base && scratch && F >= ENV_ACC_MIN_F && env_h <= 32767 && env_w <= 65535 && !getenv("IA_ENV_GRAD_ATOMIC")) {
        const int rows = ENV_ACC_LDS / (env_w * 3 * (int)sizeof(float));
        TH = rows - 1;
        n_bands = TH >= 1 ? (env_h + TH - 1) / TH : 0;
        if (TH >= 1 && n_bands <= 32 && (reinterpret_cast<uintptr_t>(scratch) & 15) == 0) {
            env_bwd_layout(scratch, scratch_bytes, F, &w);
            if (w.fits) { rec_idx = w.rec_idx; rec_w = w.rec_w; rec_g = w.rec_g; }
        }
    }
    if (mode == 0)
        pbr_light_bwd_kernel<0><<<grid, THREADS, 0, s>>>(F, inv_pdf, normal, albedo, roughness, metallic, view_dirs, out_dirs,
            transmittance, indirect_rgb, e, w2s_rot, g_Lo, g_Lo_diff, g_Lo_spec, g_normal, g_albedo, g_roughness, g_metallic, g_env_base,
            rec_idx, rec_w, rec_g);
    else
        pbr_light_bwd_kernel<1><<<grid, THREADS, 0, s>>>(F, inv_pdf, normal, albedo, roughness, metallic, view_dirs, out_dirs,
            transmittance, indirect_rgb, e, w2s_rot, g_Lo, g_Lo_diff, g_Lo_spec, g_normal, g_albedo, g_roughness, g_metallic, g_env_base,
            rec_idx, rec_w, rec_g);
    if (rec_idx) {
        static bool attr = false;
        if (!attr) {
            (void)hipFuncSetAttribute((const void*)env_band_accumulate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ENV_ACC_LDS);
            (void)hipGetLastError();
            attr = true;
        }
        const int rows64 = ENV_ACC64_LDS / (env_w * 3 * (int)sizeof(unsigned long long));
        const int TH64 = rows64 - 1, n_bands64 = TH64 >= 1 ? (env_h + TH64 - 1) / TH64 : 0;
        const bool fixed = !getenv("IA_ENV_GRAD_UNBINNED") && TH64 >= 1 && n_bands64 <= 32 && (size_t)env_h * env_w <= ENV_FIXED_MAX_TEXELS &&
                           F < ((int64_t)1 << 31) - ENV_TILE;
        if (!fixed) {
            const int n_ranges = 16;
            const size_t lds = (size_t)(TH + 1) * env_w * 3 * sizeof(float);
            env_band_accumulate_kernel<<<8 * n_bands * (n_ranges / 8), ENV_ACC_THREADS, lds, s>>>(F, rec_idx, rec_w, rec_g, env_h, env_w, TH,
                                                                                                    n_bands, n_ranges, g_env_base);
        } else {
            static bool attr64 = false;
            if (!attr64) {
                (void)hipFuncSetAttribute((const void*)env_band_accumulate_binned_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ENV_ACC64_LDS);
                (void)hipGetLastError();
                attr64 = true;
            }
            const int n_tiles = (int)((F + ENV_TILE - 1) / ENV_TILE);
            EnvRec* sorted = w.sorted;
            int32_t *counts = w.counts, *offs = w.offs, *total = w.total;
            uint32_t* gmax = w.gmax;
            void* scan_tmp = w.scan_tmp;
            unsigned long long* acc64 = w.acc64;
            const int64_t n_img = (int64_t)env_h * env_w * 3;
            int fx_shift = 62;                                          // 62 - ceil(log2 F): see env_fixed_scale
            for (int64_t f = 1; f < F; f <<= 1) fx_shift--;
            (void)hipMemsetAsync(gmax, 0, 4, s);
            (void)hipMemsetAsync(acc64, 0, (size_t)n_img * 8, s);
            env_bin_count_kernel<<<n_tiles, ENV_ACC_THREADS, 0, s>>>(F, rec_idx, rec_g, TH64, n_bands64, n_tiles, counts, gmax);
            const int rc = ia_exclusive_scan_i32(counts, offs, total, (int64_t)n_bands64 * n_tiles, scan_tmp, stream);
            if (rc != IA_OK) return rc;
            env_bin_scatter_kernel<<<n_tiles, ENV_ACC_THREADS, 0, s>>>(F, rec_idx, rec_w, rec_g, TH64, n_bands64, n_tiles, offs, sorted);
            const size_t lds64 = (size_t)(TH64 + 1) * env_w * 3 * sizeof(unsigned long long);
            env_band_accumulate_binned_kernel<<<256 + n_bands64, ENV_ACC_THREADS, lds64, s>>>(sorted, offs, total, n_tiles, env_h, env_w, TH64,
                                                                                              n_bands64, gmax, fx_shift, acc64);
            env_fixed_finish_kernel<<<ia::cdiv(n_img, THREADS), THREADS, 0, s>>>(n_img, acc64, gmax, fx_shift, g_env_base);
        }
    }
    return ia::check_launch("ia_pbr_shade_bwd");
}

IA_EXPORT int ia_pbr_light_shade(int64_t F, const float* normal, const float* albedo, const float* roughness,
                                 const float* metallic, const float* view_dirs, const float* light_dirs,
                                 const float* transmittance, const float* indirect_rgb, const float* env_base,
                                 const float* env_pmf, int env_h, int env_w, const float* w2s_rot, float* Lo,
                                 float* Lo_diff, float* Lo_spec, ia_stream_t stream)
{
    return ia_pbr_shade(0, F, normal, albedo, roughness, metallic, view_dirs, light_dirs, transmittance, indirect_rgb, nullptr,
                        env_base, env_pmf, env_h, env_w, w2s_rot, Lo, Lo_diff, Lo_spec, nullptr, stream);
}

IA_EXPORT int ia_brdf_sample(int64_t F, const float* normal, const float* view_dirs, const float* roughness, const float* u,
                             float* out_dirs, ia_stream_t stream)
{
    if (F == 0) return IA_OK;
    brdf_sample_kernel<<<ia::cdiv(F, THREADS), THREADS, 0, (hipStream_t)stream>>>(F, normal, view_dirs, roughness, u, out_dirs);
    return ia::check_launch("ia_brdf_sample");
}

IA_EXPORT int ia_brdf_pdf(int64_t F, const float* normal, const float* view_dirs, const float* out_dirs, const float* roughness,
                          float* pdf, ia_stream_t stream)
{
    if (F == 0) return IA_OK;
    brdf_pdf_kernel<<<ia::cdiv(F, THREADS), THREADS, 0, (hipStream_t)stream>>>(F, normal, view_dirs, out_dirs, roughness, pdf);
    return ia::check_launch("ia_brdf_pdf");
}

IA_EXPORT int ia_envlight_eval(int64_t n, const float* dirs_world, const float* env_base, const float* env_pmf,
                               int env_h, int env_w, float* rgb, float* pdf, ia_stream_t stream)
{
    if (n == 0) return IA_OK;
    EnvMap e{env_base, env_pmf, env_h, env_w};
    env_eval_kernel<<<ia::cdiv(n, THREADS), THREADS, 0, (hipStream_t)stream>>>(n, dirs_world, e, rgb, pdf);
    return ia::check_launch("ia_envlight_eval");
}

IA_EXPORT int ia_transform_dirs_s2w(int64_t n, const float* dirs_smpl, const float* w2s_rot, float* dirs_world, ia_stream_t stream)
{
    if (n == 0) return IA_OK;
    EnvMap e{nullptr, nullptr, 1, 1};
    env_background_kernel<<<ia::cdiv(n, THREADS), THREADS, 0, (hipStream_t)stream>>>(n, dirs_smpl, w2s_rot, e, nullptr, dirs_world);
    return ia::check_launch("ia_transform_dirs_s2w");
}

IA_EXPORT int ia_envlight_background(int64_t n, const float* rays_d_smpl, const float* w2s_rot, const float* env_base, int env_h, int env_w,
                                     float* out, ia_stream_t stream)
{
    if (n == 0) return IA_OK;
    IA_REQUIRE(env_h > 0 && env_w > 0, "environment map must be non-empty");
    EnvMap e{env_base, nullptr, env_h, env_w};
    env_background_kernel<<<ia::cdiv(n, THREADS), THREADS, 0, (hipStream_t)stream>>>(n, rays_d_smpl, w2s_rot, e, out, nullptr);
    return ia::check_launch("ia_envlight_background");
}

IA_EXPORT int ia_envlight_background_bwd(int64_t n, const float* rays_d_smpl, const float* w2s_rot, const float* g_out, int env_h, int env_w,
                                         float* g_base, int64_t* acc /*[H,W,3]*/, uint32_t* gmax /*[1]*/, ia_stream_t stream)
{
    if (n == 0) return IA_OK;
    IA_REQUIRE(env_h > 0 && env_w > 0, "environment map must be non-empty");
    IA_REQUIRE(n < ((int64_t)1 << 40), "ia_envlight_background_bwd: n must stay below 2^40");
    IA_REQUIRE(g_base && acc && gmax, "g_base [H,W,3] float, acc [H,W,3] int64 and gmax [1] uint32 are required");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_img = (int64_t)env_h * env_w * 3;
    int fx_shift = 62;                                          // 62 - ceil(log2 n): see env_fixed_scale
    for (int64_t f = 1; f < n; f <<= 1) fx_shift--;
    (void)hipMemsetAsync(gmax, 0, 4, s);
    (void)hipMemsetAsync(acc, 0, (size_t)n_img * 8, s);
    EnvMap e{nullptr, nullptr, env_h, env_w};
    unsigned long long* acc64 = reinterpret_cast<unsigned long long*>(acc);
    env_absmax_kernel<<<ia::cdiv(3 * n, THREADS), THREADS, 0, s>>>(3 * n, g_out, gmax);
    env_background_bwd_kernel<<<ia::cdiv(n, THREADS), THREADS, 0, s>>>(n, rays_d_smpl, w2s_rot, e, g_out, gmax, fx_shift, acc64);
    env_fixed_finish_kernel<<<ia::cdiv(n_img, THREADS), THREADS, 0, s>>>(n_img, acc64, gmax, fx_shift, g_base);
    return ia::check_launch("ia_envlight_background_bwd");
}

IA_EXPORT int ia_scatterer_sample(int64_t F, int lobes, const float* normal, const float* wi, const float* alpha, const float* u,
                                  float* wo, ia_stream_t stream)
{
    if (F == 0) return IA_OK;
    IA_REQUIRE(lobes >= 1 && lobes <= 4, "lobes: 1 Lambertian, 2 GGX, 3 MultiLobe, 4 Mirror");
    scatterer_sample_kernel<<<ia::cdiv(F, THREADS), THREADS, 0, (hipStream_t)stream>>>(F, lobes, normal, wi, alpha, u, wo);
    return ia::check_launch("ia_scatterer_sample");
}

IA_EXPORT int ia_scatterer_pdf(int64_t F, int lobes, const float* normal, const float* wi, const float* wo, const float* alpha,
                               float* pdf, ia_stream_t stream)
{
    if (F == 0) return IA_OK;
    IA_REQUIRE(lobes >= 1 && lobes <= 4, "lobes: 1 Lambertian, 2 GGX, 3 MultiLobe, 4 Mirror");
    scatterer_pdf_kernel<<<ia::cdiv(F, THREADS), THREADS, 0, (hipStream_t)stream>>>(F, lobes, normal, wi, wo, alpha, pdf);
    return ia::check_launch("ia_scatterer_pdf");
}

IA_EXPORT int ia_scatterer_eval(int64_t F, int lobes, const float* normal, const float* wi, const float* wo, const float* alpha,
                                const float* albedo, const float* metallic, float* diff, float* spec, ia_stream_t stream)
{
    if (F == 0) return IA_OK;
    IA_REQUIRE(lobes >= 1 && lobes <= 4, "lobes: 1 Lambertian, 2 GGX, 3 MultiLobe, 4 Mirror");
    scatterer_eval_kernel<<<ia::cdiv(F, THREADS), THREADS, 0, (hipStream_t)stream>>>(F, lobes, normal, wi, wo, alpha, albedo, metallic,
                                                                                    diff, spec);
    return ia::check_launch("ia_scatterer_eval");
}
