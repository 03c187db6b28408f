/* mc_harness.c -- host replay of the PRODUCT's marching-cubes arithmetic (intrinsicavatar_amd/csrc/mc_math.h).
 *
 * mcubes.hip wraps the functions of that header in its count / emit / face kernels.  This file runs the same extraction as plain
 * loops in the stated order (vertices by owning point then axis, faces by cell then table order) so that tests/test_mesh_cpu.py can
 * check the mesh's properties without a GPU and tests/test_gpu_mesh.py can hold the kernels to it bit for bit.
 * Built by the tests with gcc -O2 -ffp-contract=off. */
#include <stdlib.h>
#include "../intrinsicavatar_amd/csrc/mc_math.h"

#define API __attribute__((visibility("default")))

static int point_mask(const float* L, int nx, int ny, int nz, int i, int j, int k, float thr)
{
    const int64_t p = ((int64_t)i * ny + j) * nz + k, syz = (int64_t)ny * nz;
    const int hx = i + 1 < nx, hy = j + 1 < ny, hz = k + 1 < nz;
    return ia_mc_owned_mask(L[p], hx ? L[p + syz] : 0.f, hy ? L[p + nz] : 0.f, hz ? L[p + 1] : 0.f, hx, hy, hz, thr);
}

static int cell_cube(const float* L, int ny, int nz, int i, int j, int k, float thr)
{
    float c[8];
    for (int b = 0; b < 8; b++) {
        const int o = ia_mc_corner_xyz[b];
        c[b] = L[((int64_t)(i + (o & 1)) * ny + j + ((o >> 1) & 1)) * nz + k + ((o >> 2) & 1)];
    }
    return ia_mc_cube_index(c, thr);
}

/* counts: n_verts, n_tris */
API void mc_h_count(int nx, int ny, int nz, const float* L, float thr, int64_t* counts)
{
    int64_t nv = 0, nt = 0;
    for (int i = 0; i < nx; i++)
        for (int j = 0; j < ny; j++)
            for (int k = 0; k < nz; k++) {
                nv += __builtin_popcount(point_mask(L, nx, ny, nz, i, j, k, thr));
                if (i + 1 < nx && j + 1 < ny && k + 1 < nz) nt += ia_mc_n_tri(cell_cube(L, ny, nz, i, j, k, thr));
            }
    counts[0] = nv;
    counts[1] = nt;
}

/* box: vmin xyz, vmax xyz.  v_pos [n_verts, 3] float, faces [n_tris, 3] int64 */
API int mc_h_fill(int nx, int ny, int nz, const float* L, float thr, const float* box, float* v_pos, int64_t* faces)
{
    const int64_t N = (int64_t)nx * ny * nz, syz = (int64_t)ny * nz;
    int64_t* first = (int64_t*)malloc(sizeof(int64_t) * (size_t)N);
    if (!first) return -1;
    int64_t nv = 0, nt = 0;
    for (int i = 0; i < nx; i++)
        for (int j = 0; j < ny; j++)
            for (int k = 0; k < nz; k++) {
                const int64_t p = ((int64_t)i * ny + j) * nz + k;
                const int m = point_mask(L, nx, ny, nz, i, j, k, thr);
                first[p] = nv;
                const int idx[3] = {i, j, k}, n[3] = {nx, ny, nz};
                const int64_t stride[3] = {syz, nz, 1};
                for (int a = 0; a < 3; a++) {
                    if (!(m >> a & 1)) continue;
                    for (int c = 0; c < 3; c++) {
                        const float coord = c == a ? ia_mc_edge_coord(idx[a], L[p], L[p + stride[a]], thr) : (float)idx[c];
                        v_pos[3 * nv + c] = ia_mc_scale(coord, n[c], box[c], box[3 + c]);
                    }
                    nv++;
                }
            }
    for (int i = 0; i + 1 < nx; i++)
        for (int j = 0; j + 1 < ny; j++)
            for (int k = 0; k + 1 < nz; k++) {
                const int cube = cell_cube(L, ny, nz, i, j, k, thr);
                const int ntri = ia_mc_n_tri(cube);
                for (int t = 0; t < ntri; t++) {
                    int64_t id[3];
                    for (int e = 0; e < 3; e++) {
                        const int edge = ia_mc_tri_table[cube][3 * t + e];
                        const int o = ia_mc_corner_xyz[ia_mc_edge_owner[edge]];
                        const int qi = i + (o & 1), qj = j + ((o >> 1) & 1), qk = k + ((o >> 2) & 1);
                        const int64_t q = ((int64_t)qi * ny + qj) * nz + qk;
                        id[e] = first[q] + ia_mc_axis_rank(point_mask(L, nx, ny, nz, qi, qj, qk, thr), ia_mc_edge_axis[edge]);
                    }
                    faces[3 * nt + 0] = id[0];
                    faces[3 * nt + 1] = id[IA_MC_FLIP ? 2 : 1];
                    faces[3 * nt + 2] = id[IA_MC_FLIP ? 1 : 2];
                    nt++;
                }
            }
    free(first);
    return 0;
}
