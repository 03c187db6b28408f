// data_harness.c -- host replay of the training-batch arithmetic with the product's own functions
// (intrinsicavatar_amd/csrc/data_math.h, compiled as C by gcc with -ffp-contract=off).  Loaded through ctypes by tests/test_data_cpu.py.
#include <stddef.h>

#include "../intrinsicavatar_amd/csrc/data_math.h"

#define EXPORT __attribute__((visibility("default")))

// in, out_min, out_max [outer, len, inner]
EXPORT void data_h_window(int64_t outer, int64_t len, int64_t inner, int k, const float* in, float* out_min, float* out_max)
{
    for (int64_t o = 0; o < outer; o++)
        for (int64_t l = 0; l < len; l++)
            for (int64_t i = 0; i < inner; i++) {
                int64_t lo, hi;
                ia_data_window_range(l, len, k, &lo, &hi);
                const int64_t at = (o * len + l) * inner + i;
                ia_data_minmax(in + o * len * inner + i, lo, hi, inner, out_min + at, out_max + at);
            }
}

EXPORT void data_h_pick(int64_t count, const int64_t* words, int64_t n, int64_t* out)
{
    for (int64_t j = 0; j < count; j++) out[j] = ia_data_pick(words[j], n);
}

EXPORT void data_h_u8_table(float* out /*[256]*/)
{
    for (int v = 0; v < 256; v++) out[v] = ia_data_u8((uint8_t)v);
}

EXPORT int data_h_is_edge(float mask_i, float mask_o) { return ia_data_is_edge(mask_i, mask_o); }

// pixels [n] or NULL (pixel j of row j)
EXPORT void data_h_rays(int64_t n, const int64_t* pixels, int W, const double* cam, float* rays_o, float* rays_d)
{
    for (int64_t j = 0; j < n; j++) ia_data_ray(pixels ? pixels[j] : j, W, cam, rays_o + 3 * j, rays_d + 3 * j);
}
