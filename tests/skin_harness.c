// skin_harness.c -- host replay of every stage of the deformer construction with the product's own arithmetic
// (intrinsicavatar_amd/csrc/skin_math.h, compiled as C by gcc with -ffp-contract=off).  Loaded through ctypes by
// tests/test_skinning_cpu.py and tests/test_gpu_skinning.py; the control flow of the k-NN is the kernel's (fill the list with the
// first K vertices, scan the rest in index order, replace the last entry on a smaller d2, rescan, selection sort).
#include <stdlib.h>

#include "../intrinsicavatar_amd/csrc/skin_math.h"

#define EXPORT __attribute__((visibility("default")))

EXPORT float skin_h_linspace(int i, int steps) { return ia_skin_linspace(i, steps); }

EXPORT void skin_h_grid_points(int D, int H, int W, float ratio, float scale, const float* offset, float* out)
{
    for (int d = 0; d < D; d++)
        for (int h = 0; h < H; h++)
            for (int w = 0; w < W; w++) ia_skin_grid_point(d, h, w, D, H, W, ratio, scale, offset, out + 3 * (((int64_t)d * H + h) * W + w));
}

EXPORT int skin_h_knn(int64_t P, int V, int K, const float* p1, const float* p2, float* d2, int32_t* idx)
{
    if (K < 1 || K > IA_KNN_MAX_K || V < K) return 1;
    for (int64_t p = 0; p < P; p++) {
        const float px = p1[3 * p], py = p1[3 * p + 1], pz = p1[3 * p + 2];
        float* md = d2 + p * K;
        int32_t* mi = idx + p * K;
        for (int k = 0; k < K; k++) {
            md[k] = ia_knn_d2(px, py, pz, p2[3 * k], p2[3 * k + 1], p2[3 * k + 2]);
            mi[k] = k;
        }
        float wd;
        int32_t wi;
        int ws;
        ia_knn_rescan(md, mi, 1, K, &wd, &wi, &ws);
        for (int v = K; v < V; v++) {
            const float d = ia_knn_d2(px, py, pz, p2[3 * v], p2[3 * v + 1], p2[3 * v + 2]);
            if (d < wd) {
                md[ws] = d;
                mi[ws] = v;
                ia_knn_rescan(md, mi, 1, K, &wd, &wi, &ws);
            }
        }
        ia_knn_sort(md, mi, 1, K, wd, wi, ws);
    }
    return 0;
}

EXPORT void skin_h_blend(int64_t P, int K, const float* d2, const int32_t* idx, const float* weights, float* out)
{
    for (int64_t p = 0; p < P; p++) ia_skin_blend_row(d2 + p * K, idx + p * K, K, weights, out + p, P);
}

EXPORT void skin_h_smooth(int D, int H, int W, const float* src, float* dst)
{
    for (int d = 0; d < D; d++)
        for (int h = 0; h < H; h++)
            for (int w = 0; w < W; w++) ia_skin_smooth_voxel(src, dst, d, h, w, D, H, W);
}
