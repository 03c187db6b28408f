// lbs_harness.c -- host replay of forward skinning and of the vertex normals with the product's own arithmetic
// (intrinsicavatar_amd/csrc/lbs_math.h, compiled as C by gcc with -ffp-contract=off).  Loaded through ctypes by tests/test_lbs_cpu.py and
// tests/test_gpu_lbs.py.  The control flow of the normals is the kernels': count the face corners per vertex, exclusive scan, fill the
// lists (here in DESCENDING face order, so that the per-vertex sort has work to do), sort each list, sum in ascending face index.
// With -DLBS_HARNESS_MAIN it is a stand-alone program (a small self-check, for a sanitizer build).
#include <stdlib.h>
#include <string.h>

#include "../intrinsicavatar_amd/csrc/lbs_math.h"

#define EXPORT __attribute__((visibility("default")))

// w [P,24], xd [P,3], R [P,9]: each may be NULL
EXPORT void lbs_h_forward(int64_t P, const float* xc, const float* grid, int D, int H, int W, const float* offset, const float* scale,
                          const float* tfs, float* w, float* xd, float* R)
{
    for (int64_t p = 0; p < P; p++) {
        float row[IA_LBS_BONES], T[12];
        ia_lbs_weights(xc + 3 * p, grid, D, H, W, offset, scale, row);
        if (w) memcpy(w + IA_LBS_BONES * p, row, sizeof(row));
        if (!xd && !R) continue;
        ia_lbs_blend(row, tfs, T);
        for (int r = 0; r < 3 && xd; r++) xd[3 * p + r] = ia_lbs_apply(T, xc + 3 * p, r);
        for (int e = 0; e < 9 && R; e++) R[9 * p + e] = T[4 * (e / 3) + e % 3];
    }
}

// which corners of a point's cell carry a load: mask bit k = corner k is inside the grid; cell [3] = (x0, y0, z0)
EXPORT void lbs_h_corners(int64_t P, const float* xc, int D, int H, int W, const float* offset, const float* scale, int32_t* cell,
                          int32_t* mask)
{
    for (int64_t p = 0; p < P; p++) {
        int32_t off[8];
        float cw[8];
        const float* x = xc + 3 * p;
        ia_lbs_corners((x[0] + offset[0]) * scale[0], (x[1] + offset[1]) * scale[1], (x[2] + offset[2]) * scale[2], D, H, W, off, cw);
        int m = 0, first = -1;
        for (int k = 0; k < 8; k++) {
            if (off[k] >= 0) m |= 1 << k;
            if (off[k] >= 0 && first < 0) first = off[k];
        }
        mask[p] = m;                                           // corner 0 is always inside
        cell[3 * p] = first % W;
        cell[3 * p + 1] = (first / W) % H;
        cell[3 * p + 2] = first / (W * H);
    }
}

// offsets [V+1], lists [3T] (sorted per vertex on return), v_nrm [V,3]; returns 0, or 1 when the sizes do not fit 31 bits
EXPORT int lbs_h_vertex_normals(int64_t V, int64_t T, const float* v_pos, const int64_t* faces, int32_t* offsets, int32_t* lists,
                                float* v_nrm)
{
    if (V < 0 || T < 0 || V >= INT32_MAX || 3 * T > INT32_MAX) return 1;
    int32_t* cursor = (int32_t*)calloc((size_t)V + 1, sizeof(int32_t));
    if (!cursor) return 1;
    for (int64_t v = 0; v <= V; v++) offsets[v] = 0;
    for (int64_t t = 0; t < T; t++) {
        if (!ia_mesh_face_ok(faces + 3 * t, V)) continue;
        for (int c = 0; c < 3; c++) offsets[faces[3 * t + c]]++;
    }
    int32_t run = 0;
    for (int64_t v = 0; v <= V; v++) {
        const int32_t n = offsets[v];
        offsets[v] = run;
        run += n;
    }
    for (int64_t t = T - 1; t >= 0; t--) {
        if (!ia_mesh_face_ok(faces + 3 * t, V)) continue;
        for (int c = 0; c < 3; c++) {
            const int64_t v = faces[3 * t + c];
            lists[offsets[v] + cursor[v]++] = (int32_t)t;
        }
    }
    for (int64_t v = 0; v < V; v++) {
        const int n = offsets[v + 1] - offsets[v];
        ia_mesh_sort_faces(lists + offsets[v], n);
        ia_mesh_vertex_normal(v_pos, V, faces, T, lists + offsets[v], n, v_nrm + 3 * v);
    }
    free(cursor);
    return 0;
}

#ifdef LBS_HARNESS_MAIN
#include <stdio.h>

int main(void)
{
    enum { D = 2, H = 3, W = 4, P = 64 };
    const int chan = D * H * W;
    float* grid = (float*)malloc(sizeof(float) * IA_LBS_BONES * chan);
    for (int i = 0; i < IA_LBS_BONES * chan; i++) grid[i] = 1.0f / IA_LBS_BONES;
    float tfs[IA_LBS_BONES * 16];
    for (int j = 0; j < IA_LBS_BONES; j++)
        for (int e = 0; e < 16; e++) tfs[16 * j + e] = (e % 5 == 0) ? 1.0f : 0.0f;
    const float offset[3] = {0.1f, -0.2f, 0.05f}, scale[3] = {0.9f, 1.1f, 3.6f};
    float* xc = (float*)malloc(sizeof(float) * 3 * P);
    for (int i = 0; i < 3 * P; i++) xc[i] = -2.0f + 4.0f * (float)((i * 37) % 101) / 100.0f;      // inside and outside the box
    xc[0] = NAN;
    float *w = (float*)malloc(sizeof(float) * 24 * P), *xd = (float*)malloc(sizeof(float) * 3 * P), *R = (float*)malloc(sizeof(float) * 9 * P);
    int32_t *cell = (int32_t*)malloc(sizeof(int32_t) * 3 * P), *mask = (int32_t*)malloc(sizeof(int32_t) * P);
    lbs_h_forward(P, xc, grid, D, H, W, offset, scale, tfs, w, xd, R);
    lbs_h_forward(P, xc, grid, D, H, W, offset, scale, NULL, w, NULL, NULL);
    lbs_h_corners(P, xc, D, H, W, offset, scale, cell, mask);
    int bad = 0;
    for (int p = 1; p < P; p++) {
        float s = 0.0f;
        for (int j = 0; j < 24; j++) s += w[24 * p + j];
        if (fabsf(s - 1.0f) > 1e-5f) bad++;
        for (int e = 0; e < 3; e++)
            if (fabsf(xd[3 * p + e] - xc[3 * p + e]) > 1e-5f * 4.0f) bad++;
        if (!(mask[p] & 1) || cell[3 * p] < 0 || cell[3 * p] >= W || cell[3 * p + 1] >= H || cell[3 * p + 2] >= D) bad++;
    }
    // a tetrahedron, one face with an index out of range, one degenerate face
    const float v_pos[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    const int64_t faces[18] = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3, 0, 1, 7, 2, 2, 3};
    int32_t offsets[5], lists[18];
    float nrm[12];
    if (lbs_h_vertex_normals(4, 6, v_pos, faces, offsets, lists, nrm) != 0) bad++;
    if (offsets[4] != 15) bad++;
    for (int v = 0; v < 4; v++) {
        const float l = sqrtf(nrm[3 * v] * nrm[3 * v] + nrm[3 * v + 1] * nrm[3 * v + 1] + nrm[3 * v + 2] * nrm[3 * v + 2]);
        if (fabsf(l - 1.0f) > 1e-6f) bad++;
        for (int i = offsets[v] + 1; i < offsets[v + 1]; i++)
            if (lists[i - 1] > lists[i]) bad++;
    }
    if (lbs_h_vertex_normals(3, 0, v_pos, faces, offsets, lists, nrm) != 0 || nrm[0] != 0.0f) bad++;
    free(grid); free(xc); free(w); free(xd); free(R); free(cell); free(mask);
    printf(bad ? "lbs_harness FAILED (%d)\n" : "lbs_harness OK\n", bad);
    return bad != 0;
}
#endif
