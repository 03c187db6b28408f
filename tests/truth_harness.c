// truth_harness.c -- host replay of the ground-truth-frame arithmetic with the product's own functions
// (intrinsicavatar_amd/csrc/data_math.h, compiled as C by gcc with -ffp-contract=off).  Loaded through ctypes by tests/test_truth_cpu.py
// and tests/golden/make_golden_truth.py.
#include <stddef.h>

#include "../intrinsicavatar_amd/csrc/data_math.h"

#define EXPORT __attribute__((visibility("default")))

EXPORT void truth_h_decode_tables(float* albedo /*[256]*/, float* normal /*[256]*/)
{
    for (int v = 0; v < 256; v++) {
        albedo[v] = ia_data_u8((uint8_t)v);
        normal[v] = ia_data_normal_u8((uint8_t)v);
    }
}

EXPORT int truth_h_mask_counts(float m) { return ia_data_mask_counts(m); }

// masks [F,H,W] -> rect [F,4]: the bounds taken in pixel order, as one lane of the kernel takes its share
EXPORT void truth_h_valid_rect(int64_t F, int H, int W, const float* masks, int k, int32_t* rect)
{
    for (int64_t f = 0; f < F; f++) {
        int xmin = W, ymin = H, xmax = -1, ymax = -1;
        for (int64_t p = 0; p < (int64_t)H * W; p++) {
            if (!ia_data_mask_counts(masks[f * H * W + p])) continue;
            const int x = (int)(p % W), y = (int)(p / W);
            xmin = x < xmin ? x : xmin;
            ymin = y < ymin ? y : ymin;
            xmax = x > xmax ? x : xmax;
            ymax = y > ymax ? y : ymax;
        }
        ia_data_valid_rect(xmin, ymin, xmax, ymax, H, W, k, rect + 4 * f);
    }
}

// valid [H*W] bytes 0 / 1 of one frame's rectangle
EXPORT void truth_h_valid_mask(int H, int W, const int32_t* rect, uint8_t* valid)
{
    for (int64_t p = 0; p < (int64_t)H * W; p++) valid[p] = (uint8_t)ia_data_in_rect(p, W, rect);
}

// in [F,H,W,C] -> out [F,H/s,W/s,C]
EXPORT void truth_h_downscale_u8(int64_t F, int H, int W, int Cn, int s, const uint8_t* in, uint8_t* out)
{
    const int Ho = H / s, Wo = W / s;
    for (int64_t f = 0; f < F; f++)
        for (int64_t yo = 0; yo < Ho; yo++)
            for (int64_t xo = 0; xo < Wo; xo++)
                for (int c = 0; c < Cn; c++) {
                    const int64_t x0 = ia_data_center_src(xo, s), y0 = ia_data_center_src(yo, s);
                    const int64_t at = ((f * H + y0) * W + x0) * Cn + c, row = (int64_t)W * Cn;
                    out[((f * Ho + yo) * Wo + xo) * Cn + c] = ia_data_center_u8(in[at], in[at + Cn], in[at + row], in[at + row + Cn]);
                }
}

EXPORT void truth_h_downscale_f32(int64_t F, int H, int W, int s, const float* in, float* out)
{
    const int Ho = H / s, Wo = W / s;
    for (int64_t f = 0; f < F; f++)
        for (int64_t yo = 0; yo < Ho; yo++)
            for (int64_t xo = 0; xo < Wo; xo++) {
                const int64_t x0 = ia_data_center_src(xo, s), y0 = ia_data_center_src(yo, s);
                const int64_t at = (f * H + y0) * W + x0;
                out[(f * Ho + yo) * Wo + xo] = ia_data_center_f32(in[at], in[at + 1], in[at + W], in[at + W + 1]);
            }
}

// every pixel of an H x W frame in order
EXPORT void truth_h_rays(int64_t n, int W, const double* cam, float* rays_o, float* rays_d)
{
    for (int64_t j = 0; j < n; j++) ia_data_ray(j, W, cam, rays_o + 3 * j, rays_d + 3 * j);
}
