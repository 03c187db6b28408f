// skin_math.h -- the arithmetic of the skinning-weight grid a deformer is built from (ForwardDeformer.switch_to_explicit +
// query_weights_smpl, models/deformers/fast_snarf/deformer_torch.py:139-253; pytorch3d's knn_points as its CPU implementation
// lib/pytorch3d/cuda/knn_cpu.cpp:13-69 defines it).  Compiles as C (gcc: tests/skin_harness.c replays every stage on the host) and as
// HIP device code (skinning.hip wraps these functions in its kernels), so both evaluate the same expressions.
//
// Conventions (DESIGN.md "Deformer construction"):
//   * voxel centres: C order over [D, H, W] (W fastest), x from W, y from H, z from D; torch.linspace(-1, 1, n)'s two-sided formula,
//     then z / ratio, * scale, + offset, one float32 rounding each.
//   * k-NN: d2 = ((dx*dx + dy*dy) + dz*dz) in float32; the result is the K smallest pairs under the lexicographic order (d2, index),
//     ascending in that order: equal distances are ordered by vertex index.
//   * blend: dist = clamp(sqrt(d2), 1e-4, 1), ws = 1 / dist, ws /= (sum over k, ascending k); row = sum over k of ws_k * W[idx_k],
//     ascending k, starting from the k = 0 product.
//   * smoothing sweep: mean = ((((( d+1 + d-1 ) + h+1 ) + h-1 ) + w+1 ) + w-1 ) / 6 from the OLD buffer, interior voxels get
//     (w - mean) * 0.7 + mean, border voxels stay; then every voxel is divided by its 24-channel sum (ascending channel).
//
// Must be built without FMA contraction / fast-math.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define IA_SKIN_FN __device__ __forceinline__
#else
#define IA_SKIN_FN static inline
#endif

#define IA_SKIN_CHANNELS 24
#define IA_KNN_MAX_K 32

// element i of torch.linspace(-1, 1, steps) in float32: start + i * step below the midpoint, end - (steps - 1 - i) * step from it on
IA_SKIN_FN float ia_skin_linspace(int i, int steps)
{
    const float start = -1.0f, end = 1.0f;
    if (steps == 1) return start;
    const float step = (end - start) / (float)(steps - 1);
    if (i < steps / 2) {
        const float m = step * (float)i;
        return start + m;
    }
    const float m = step * (float)(steps - i - 1);
    return end - m;
}

// denormalize() of switch_to_explicit on one coordinate triple: z /= ratio, then * scale, then + offset
IA_SKIN_FN void ia_skin_grid_point(int d, int h, int w, int D, int H, int W, float ratio, float scale, const float offset[3], float out[3])
{
    const float x = ia_skin_linspace(w, W), y = ia_skin_linspace(h, H);
    const float z = ia_skin_linspace(d, D) / ratio;
    const float sx = x * scale, sy = y * scale, sz = z * scale;
    out[0] = sx + offset[0];
    out[1] = sy + offset[1];
    out[2] = sz + offset[2];
}

IA_SKIN_FN float ia_knn_d2(float px, float py, float pz, float vx, float vy, float vz)
{
    const float dx = px - vx, dy = py - vy, dz = pz - vz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float s = xx + yy;
    return s + zz;
}

// (da, ia) comes after (db, ib) in the order of the result
IA_SKIN_FN int ia_knn_after(float da, int32_t ia, float db, int32_t ib) { return da > db || (da == db && ia > ib); }

// the last entry, in the order of the result, of the n list slots ld[k * stride], li[k * stride]
IA_SKIN_FN void ia_knn_rescan(const float* ld, const int32_t* li, int stride, int n, float* wd, int32_t* wi, int* ws)
{
    float bd = ld[0];
    int32_t bi = li[0];
    int bs = 0;
    for (int k = 1; k < n; k++) {
        const float d = ld[k * stride];
        const int32_t i = li[k * stride];
        if (ia_knn_after(d, i, bd, bi)) {
            bd = d;
            bi = i;
            bs = k;
        }
    }
    *wd = bd;
    *wi = bi;
    *ws = bs;
}

// in-place selection sort of the n slots into ascending (d2, index) order; (wd, wi, ws) is the current last entry of all n
IA_SKIN_FN void ia_knn_sort(float* ld, int32_t* li, int stride, int n, float wd, int32_t wi, int ws)
{
    for (int k = n - 1; k > 0; k--) {
        const float td = ld[k * stride];
        const int32_t ti = li[k * stride];
        ld[k * stride] = wd;
        li[k * stride] = wi;
        ld[ws * stride] = td;
        li[ws * stride] = ti;
        ia_knn_rescan(ld, li, stride, k, &wd, &wi, &ws);
    }
}

IA_SKIN_FN float ia_skin_inv_dist(float d2)
{
    float dist = sqrtf(d2);
    dist = dist < 0.0001f ? 0.0001f : dist;
    dist = dist > 1.0f ? 1.0f : dist;
    return 1.0f / dist;
}

// one row of query_weights_smpl before the reshape: d2, idx [K] (stride 1) -> out[c * out_stride], c < 24
IA_SKIN_FN void ia_skin_blend_row(const float* d2, const int32_t* idx, int K, const float* W /*[V,24]*/, float* out, int64_t out_stride)
{
    float sum = ia_skin_inv_dist(d2[0]);
    for (int k = 1; k < K; k++) sum = sum + ia_skin_inv_dist(d2[k]);
    float acc[IA_SKIN_CHANNELS];
    for (int k = 0; k < K; k++) {
        const float ws = ia_skin_inv_dist(d2[k]) / sum;
        const float* row = W + (int64_t)idx[k] * IA_SKIN_CHANNELS;
#ifdef __HIPCC__
#pragma unroll
#endif
        for (int c = 0; c < IA_SKIN_CHANNELS; c++) {
            const float m = ws * row[c];
            acc[c] = k == 0 ? m : acc[c] + m;
        }
    }
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int c = 0; c < IA_SKIN_CHANNELS; c++) out[c * out_stride] = acc[c];
}

// one voxel of one smoothing sweep: src, dst [24, D, H, W]
IA_SKIN_FN void ia_skin_smooth_voxel(const float* src, float* dst, int d, int h, int w, int D, int H, int W)
{
    const int64_t sH = W, sD = (int64_t)H * W, sC = (int64_t)D * H * W;
    const int64_t v = (int64_t)d * sD + (int64_t)h * sH + w;
    const int interior = d > 0 && d < D - 1 && h > 0 && h < H - 1 && w > 0 && w < W - 1;
    float val[IA_SKIN_CHANNELS];
    float sum = 0.0f;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int c = 0; c < IA_SKIN_CHANNELS; c++) {
        const float* s = src + c * sC + v;
        float x = s[0];
        if (interior) {
            float m = s[sD] + s[-sD];
            m = m + s[sH];
            m = m + s[-sH];
            m = m + s[1];
            m = m + s[-1];
            m = m / 6.0f;
            const float t = (x - m) * 0.7f;
            x = t + m;
        }
        val[c] = x;
        sum = c == 0 ? x : sum + x;
    }
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int c = 0; c < IA_SKIN_CHANNELS; c++) dst[c * sC + v] = val[c] / sum;
}
