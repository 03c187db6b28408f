// data_math.h -- the arithmetic of a training batch: camera rays (make_rays, datasets/peoplesnapshot.py:19-33), the windowed minimum /
// maximum behind EdgeSampler's edge band (cv2.erode / cv2.dilate with a rectangular kernel, utils/sampler.py:27-31), the index rule of
// the samplers' draws and the u8 -> float32 image conversion (datasets/peoplesnapshot.py:126).  Compiles as C (gcc: tests/data_harness.c
// replays every function on the host) and as HIP device code (data.hip wraps these functions in its kernels), so both evaluate the same
// expressions.
//
// Conventions (DESIGN.md "Training batches"):
//   * rays: fp64 throughout.  d_c = (x, y, 1) . inv(K)^T, d_w = d_c . R^T, each a three-term sum formed left to right from separately
//     rounded products; d_w / sqrt((dx*dx + dy*dy) + dz*dz); one rounding to float32 at the end.  x = p % W, y = p / W.
//   * window: k taps at offsets -(k/2) ... k - 1 - k/2 around an element, taps outside the array ignored (OpenCV's anchor k/2 and its
//     default border value, which never wins).  The centre tap always exists, so every window is non-empty.
//   * draw: word % n on non-negative int64 words (np.random.randint(0, n) replayed from recorded words).
//   * image: float32(double(u8) / 255.0).
//
// Must be built without FMA contraction / fast-math.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define IA_DATA_FN __device__ __forceinline__
#else
#define IA_DATA_FN static inline
#endif

#define IA_WINDOW_MAX_K 64

// cam [21]: inv(K) row-major [9], R = c2w[:3,:3] row-major [9], c2w[:3,3] [3]
IA_DATA_FN void ia_data_ray(int64_t p, int W, const double* cam, float o[3], float d[3])
{
    const double x = (double)(p % W), y = (double)(p / W);
    double dc[3], dw[3];
    for (int j = 0; j < 3; j++) {
        const double a = x * cam[3 * j], b = y * cam[3 * j + 1], c = 1.0 * cam[3 * j + 2];
        const double s = a + b;
        dc[j] = s + c;
    }
    for (int j = 0; j < 3; j++) {
        const double a = dc[0] * cam[9 + 3 * j], b = dc[1] * cam[9 + 3 * j + 1], c = dc[2] * cam[9 + 3 * j + 2];
        const double s = a + b;
        dw[j] = s + c;
    }
    const double xx = dw[0] * dw[0], yy = dw[1] * dw[1], zz = dw[2] * dw[2];
    const double s = xx + yy;
    const double norm = sqrt(s + zz);
    for (int j = 0; j < 3; j++) {
        d[j] = (float)(dw[j] / norm);
        o[j] = (float)cam[18 + j];
    }
}

// first and one-past-last tap of the window around element i of an array of `len` elements
IA_DATA_FN void ia_data_window_range(int64_t i, int64_t len, int k, int64_t* lo, int64_t* hi)
{
    const int64_t a = i - k / 2, b = i + (k - 1 - k / 2) + 1;
    *lo = a < 0 ? 0 : a;
    *hi = b > len ? len : b;
}

// minimum and maximum of src[lo * stride], ..., src[(hi - 1) * stride] (lo < hi), taken in ascending order
IA_DATA_FN void ia_data_minmax(const float* src, int64_t lo, int64_t hi, int64_t stride, float* mn, float* mx)
{
    float a = src[lo * stride], b = a;
    for (int64_t t = lo + 1; t < hi; t++) {
        const float v = src[t * stride];
        a = v < a ? v : a;
        b = v > b ? v : b;
    }
    *mn = a;
    *mx = b;
}

IA_DATA_FN int64_t ia_data_pick(int64_t word, int64_t n) { return word % n; }

IA_DATA_FN float ia_data_u8(uint8_t v) { return (float)((double)v / 255.0); }

// the edge test of EdgeSampler.sample: np.where(mask_o - mask_i) on the float values
IA_DATA_FN int ia_data_is_edge(float mask_i, float mask_o) { return (mask_o - mask_i) != 0.0f; }
