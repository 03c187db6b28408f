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

// ----------------------------------------------------------------------------- ground-truth frames (datasets/rana.py, synthetichuman.py)
// Conventions (DESIGN.md "Ground-truth frames"):
//   * albedo: ia_data_u8, as rgb.  normal: ((n / 255).astype(float32) - 0.5) * 2 = (ia_data_u8(v) - 0.5f) * 2.0f, both steps in float32.
//   * valid mask: msk.astype(np.uint8) != 0.  For 0 <= m < 256 the cast truncates, so a pixel counts iff m >= 1.0f (fractions give 0).
//     A mask value outside [0, 256) (or NaN) has no defined result in numpy's cast either; here it counts iff m >= 1.0f.
//   * valid rectangle: the bounding rectangle of the counting pixels dilated by a k x k window with taps at -(k/2) ... k - 1 - k/2 is the
//     source's bounding rectangle grown by k - 1 - k/2 towards 0 and by k/2 towards the far side, clipped to the image; an empty source
//     gives (0, 0, 0, 0).  Even k is asymmetric.
//   * downscale by an even integer s (H % s == W % s == 0): cv2.resize's default INTER_LINEAR samples midway between source pixels
//     s * d + s/2 - 1 and s * d + s/2 on both axes.  u8: (a + b + c + d + 2) >> 2; float32: ((a + b) + (c + d)) * 0.25f.

IA_DATA_FN float ia_data_normal_u8(uint8_t v) { return (ia_data_u8(v) - 0.5f) * 2.0f; }

IA_DATA_FN int ia_data_mask_counts(float m) { return m >= 1.0f; }

// (xmin, ymin, xmax, ymax) of the counting pixels of an H x W mask (xmax < xmin: there is none) -> rect = (x, y, w, h)
IA_DATA_FN void ia_data_valid_rect(int xmin, int ymin, int xmax, int ymax, int H, int W, int k, int32_t rect[4])
{
    if (xmax < xmin || ymax < ymin) {
        rect[0] = rect[1] = rect[2] = rect[3] = 0;
        return;
    }
    const int near_side = k - 1 - k / 2, far_side = k / 2;
    const int x0 = xmin - near_side > 0 ? xmin - near_side : 0, y0 = ymin - near_side > 0 ? ymin - near_side : 0;
    const int x1 = xmax + far_side < W - 1 ? xmax + far_side : W - 1, y1 = ymax + far_side < H - 1 ? ymax + far_side : H - 1;
    rect[0] = x0;
    rect[1] = y0;
    rect[2] = x1 - x0 + 1;
    rect[3] = y1 - y0 + 1;
}

// valid_msk[y : y + h, x : x + w] = True, read at pixel p = y * W + x
IA_DATA_FN int ia_data_in_rect(int64_t p, int W, const int32_t rect[4])
{
    const int64_t x = p % W, y = p / W;
    return x >= rect[0] && x < (int64_t)rect[0] + rect[2] && y >= rect[1] && y < (int64_t)rect[1] + rect[3];
}

// first of the two source positions either side of the sample point of output position d (the second is the next one)
IA_DATA_FN int64_t ia_data_center_src(int64_t d, int s) { return (int64_t)s * d + s / 2 - 1; }

IA_DATA_FN uint8_t ia_data_center_u8(uint8_t a, uint8_t b, uint8_t c, uint8_t d) { return (uint8_t)(((int)a + (int)b + (int)c + (int)d + 2) >> 2); }

IA_DATA_FN float ia_data_center_f32(float a, float b, float c, float d)
{
    const float top = a + b, bottom = c + d;
    return (top + bottom) * 0.25f;
}
