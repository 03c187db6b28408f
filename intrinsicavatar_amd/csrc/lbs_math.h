// lbs_math.h -- the per-point arithmetic of forward skinning (ForwardDeformer.forward_skinning = query_weights + skinning_mask,
// models/deformers/fast_snarf/deformer_torch.py:127-137, :199-210, :213-227) and of the area-weighted vertex normals of a triangle
// mesh.  Compiles as C (gcc: tests/lbs_harness.c replays it on the host) and as HIP device code (lbs_fwd.hip and mesh_attr.hip wrap these
// functions in their kernels), so both evaluate the same expressions.
//
// Conventions (DESIGN.md "Forward skinning and mesh attributes"):
//   * sampling = grid_sample(align_corners=True, mode='bilinear', padding_mode='border') of the channel-major grid [24,D,H,W] at
//     g = (xc + offset) * scale: g.x addresses W, g.y H, g.z D; index = ((g + 1) / 2) * (n - 1), clamped to [0, n - 1]; the cell is
//     floor(index); the eight corners in the order (x0 y0 z0), (x1 y0 z0), (x0 y1 z0), (x1 y1 z0), (x0 y0 z1), ... with the weight
//     (wx * wy) * wz, wx = (x0 + 1) - ix for x0 and ix - x0 for x1; a corner past the last node carries weight 0 and is not loaded.
//     A channel's value = 0 + v0 * c0 + v1 * c1 + ... in that corner order.  A NaN coordinate samples node 0.
//   * blend: T = w_0 * tfs_0, then T = T + w_j * tfs_j in ascending j (rows 0 .. 2 of the 4 x 4 only);
//     xd_r = ((T_r0 * x + T_r1 * y) + T_r2 * z) + T_r3;  R = T[:3,:3].
//   * normals: a face adds the un-normalised (v1 - v0) x (v2 - v0) to each of its three vertices; a vertex sums its incident faces in
//     ascending face index starting from 0, then n / max(|n|, 1e-12) with |n| = sqrt((x*x + y*y) + z*z).
//
// Must be built without FMA contraction / fast-math.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define IA_LBS_FN __device__ __forceinline__
#define IA_LBS_UNROLL _Pragma("unroll")
#else
#define IA_LBS_FN static inline
#define IA_LBS_UNROLL
#endif

#define IA_LBS_BONES 24

// grid_sampler_unnormalize (align_corners) + clip_coordinates of one axis with n nodes
IA_LBS_FN float ia_lbs_index(float g, int n)
{
    const float last = (float)(n - 1);
    float c = ((g + 1.0f) / 2.0f) * last;
    c = c > 0.0f ? c : 0.0f;               // (a NaN ends at 0)
    c = c < last ? c : last;
    return c;
}

// the eight corners of the cell of g = (gx, gy, gz): off[k] = offset of corner k inside one channel [D,H,W], or -1 for a corner past
// the last node of an axis; cw[k] = its trilinear weight
IA_LBS_FN void ia_lbs_corners(float gx, float gy, float gz, int D, int H, int W, int32_t off[8], float cw[8])
{
    const float ix = ia_lbs_index(gx, W), iy = ia_lbs_index(gy, H), iz = ia_lbs_index(gz, D);
    const float fx = floorf(ix), fy = floorf(iy), fz = floorf(iz);
    const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
    const float wx[2] = {(fx + 1.0f) - ix, ix - fx};
    const float wy[2] = {(fy + 1.0f) - iy, iy - fy};
    const float wz[2] = {(fz + 1.0f) - iz, iz - fz};
    IA_LBS_UNROLL
    for (int k = 0; k < 8; k++) {
        const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
        const int x = x0 + dx, y = y0 + dy, z = z0 + dz;
        const int inside = x < W && y < H && z < D;
        off[k] = inside ? (z * H + y) * W + x : -1;
        cw[k] = (wx[dx] * wy[dy]) * wz[dz];
    }
}

IA_LBS_FN float ia_lbs_sample(const float* chan, const int32_t off[8], const float cw[8])
{
    float acc = 0.0f;
    IA_LBS_UNROLL
    for (int k = 0; k < 8; k++) {
        if (off[k] >= 0) {
            const float m = chan[off[k]] * cw[k];
            acc = acc + m;
        }
    }
    return acc;
}

// the weights of one point: grid [24,D,H,W], offset / scale [3] -> w [24]
IA_LBS_FN void ia_lbs_weights(const float* xc, const float* grid, int D, int H, int W, const float* offset, const float* scale,
                              float w[IA_LBS_BONES])
{
    const float gx = (xc[0] + offset[0]) * scale[0], gy = (xc[1] + offset[1]) * scale[1], gz = (xc[2] + offset[2]) * scale[2];
    int32_t off[8];
    float cw[8];
    ia_lbs_corners(gx, gy, gz, D, H, W, off, cw);
    const int32_t chan = D * H * W;
    IA_LBS_UNROLL
    for (int j = 0; j < IA_LBS_BONES; j++) w[j] = ia_lbs_sample(grid + (int64_t)j * chan, off, cw);
}

// rows 0 .. 2 of the blended transform: w [24], tfs [24,4,4] -> T [12] (row-major 3 x 4)
IA_LBS_FN void ia_lbs_blend(const float w[IA_LBS_BONES], const float* tfs, float T[12])
{
    IA_LBS_UNROLL
    for (int j = 0; j < IA_LBS_BONES; j++) {
        IA_LBS_UNROLL
        for (int e = 0; e < 12; e++) {
            const float m = w[j] * tfs[16 * j + e];
            T[e] = j == 0 ? m : T[e] + m;
        }
    }
}

// component r of the skinned point
IA_LBS_FN float ia_lbs_apply(const float T[12], const float* xc, int r)
{
    const float a = T[4 * r] * xc[0], b = T[4 * r + 1] * xc[1], c = T[4 * r + 2] * xc[2];
    float s = a + b;
    s = s + c;
    return s + T[4 * r + 3];
}

// ---- vertex normals ---------------------------------------------------------------------------------------------------------------
// a face is used only when its three vertex indices lie in [0, V)
IA_LBS_FN int ia_mesh_face_ok(const int64_t* face, int64_t V)
{
    return (uint64_t)face[0] < (uint64_t)V && (uint64_t)face[1] < (uint64_t)V && (uint64_t)face[2] < (uint64_t)V;
}

// un-normalised (v1 - v0) x (v2 - v0): twice the face's area along its normal
IA_LBS_FN void ia_mesh_face_cross(const float* v_pos, const int64_t* face, float n[3])
{
    const float* a = v_pos + 3 * face[0];
    const float* b = v_pos + 3 * face[1];
    const float* c = v_pos + 3 * face[2];
    const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    const float yz = e1y * e2z, zy = e1z * e2y;
    const float zx = e1z * e2x, xz = e1x * e2z;
    const float xy = e1x * e2y, yx = e1y * e2x;
    n[0] = yz - zy;
    n[1] = zx - xz;
    n[2] = xy - yx;
}

// in-place insertion sort of a vertex's face list into ascending face index
IA_LBS_FN void ia_mesh_sort_faces(int32_t* list, int n)
{
    for (int i = 1; i < n; i++) {
        const int32_t f = list[i];
        int k = i;
        while (k > 0 && list[k - 1] > f) {
            list[k] = list[k - 1];
            k--;
        }
        list[k] = f;
    }
}

// the normal of one vertex from its sorted face list (entries outside [0, T) or faces with a bad index are skipped)
IA_LBS_FN void ia_mesh_vertex_normal(const float* v_pos, int64_t V, const int64_t* faces, int64_t T, const int32_t* list, int n, float out[3])
{
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int i = 0; i < n; i++) {
        const int32_t f = list[i];
        if ((uint64_t)f >= (uint64_t)T || !ia_mesh_face_ok(faces + 3 * (int64_t)f, V)) continue;
        float c[3];
        ia_mesh_face_cross(v_pos, faces + 3 * (int64_t)f, c);
        sx = sx + c[0];
        sy = sy + c[1];
        sz = sz + c[2];
    }
    const float xx = sx * sx, yy = sy * sy, zz = sz * sz;
    float len = xx + yy;
    len = sqrtf(len + zz);
    len = len > 1e-12f ? len : 1e-12f;
    out[0] = sx / len;
    out[1] = sy / len;
    out[2] = sz / len;
}
