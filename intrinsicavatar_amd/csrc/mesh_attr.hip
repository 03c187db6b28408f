// mesh_attr.hip -- per-vertex attributes of a triangle mesh: the vertex -> incident-faces lists (CSR) and the area-weighted vertex
// normals summed over them.  No float atomics: incidences are counted with integer atomics, the caller scans the counts
// (ia_exclusive_scan_i32), the lists are filled through per-vertex cursors (integer atomics: the order inside a list depends on
// scheduling), and the normals kernel -- one vertex per lane -- sorts its own short list in place and sums in ascending face index, so
// the lists it leaves and the normals do not depend on scheduling.  A face with a vertex index outside [0, V) is ignored by all three.
// The arithmetic lives in lbs_math.h (replayed on the host by tests/lbs_harness.c).  Built with -ffp-contract=off.
#include "ia_common.h"
#include "lbs_math.h"

namespace {

__global__ __launch_bounds__(256) void vertex_faces_count_kernel(int64_t T, int64_t V, const int64_t* __restrict__ faces,
                                                                 int32_t* __restrict__ counts)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const int64_t* f = faces + 3 * t;
    if (!ia_mesh_face_ok(f, V)) return;
    atomicAdd(&counts[f[0]], 1);
    atomicAdd(&counts[f[1]], 1);
    atomicAdd(&counts[f[2]], 1);
}

__global__ __launch_bounds__(256) void vertex_faces_fill_kernel(int64_t T, int64_t V, const int64_t* __restrict__ faces,
                                                                const int32_t* __restrict__ offsets, int32_t* __restrict__ cursor,
                                                                int32_t* __restrict__ lists)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const int64_t* f = faces + 3 * t;
    if (!ia_mesh_face_ok(f, V)) return;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int64_t v = f[c];
        const int64_t slot = (int64_t)offsets[v] + atomicAdd(&cursor[v], 1);
        // offsets that are not the scan of this mesh's counts must not send a store outside the vertex's range or the list
        if (slot >= 0 && slot < (int64_t)offsets[v + 1] && slot < 3 * T) lists[slot] = (int32_t)t;
    }
}

__global__ __launch_bounds__(256) void vertex_normals_kernel(int64_t V, int64_t T, const float* __restrict__ v_pos,
                                                             const int64_t* __restrict__ faces, const int32_t* __restrict__ offsets,
                                                             int32_t* __restrict__ lists, float* __restrict__ v_nrm)
{
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int64_t b = offsets[v], e = offsets[v + 1];
    int n = 0;
    if (b >= 0 && e >= b && e <= 3 * T) n = (int)(e - b);
    int32_t* list = lists + (n > 0 ? b : 0);
    ia_mesh_sort_faces(list, n);
    float out[3];
    ia_mesh_vertex_normal(v_pos, V, faces, T, list, n, out);
    v_nrm[3 * v] = out[0];
    v_nrm[3 * v + 1] = out[1];
    v_nrm[3 * v + 2] = out[2];
}

bool mesh_ok(int64_t T, int64_t V) { return T >= 0 && V >= 0 && V < INT32_MAX && 3 * T <= INT32_MAX; }

}  // namespace

IA_EXPORT int ia_mesh_vertex_faces_count(int64_t T, int64_t V, const int64_t* faces, int32_t* counts, ia_stream_t stream)
{
    IA_REQUIRE(mesh_ok(T, V), "V and 3 * T must fit 31 bits");
    IA_REQUIRE(counts && (faces || T == 0), "null pointer");
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)(V + 1) * sizeof(int32_t), (hipStream_t)stream);
    if (e != hipSuccess) {
        ia::set_error("ia_mesh_vertex_faces_count: %s", hipGetErrorString(e));
        return IA_ERR_LAUNCH;
    }
    if (T == 0) return IA_OK;
    vertex_faces_count_kernel<<<ia::cdiv(T, 256), 256, 0, (hipStream_t)stream>>>(T, V, faces, counts);
    return ia::check_launch("ia_mesh_vertex_faces_count");
}

IA_EXPORT int ia_mesh_vertex_faces_fill(int64_t T, int64_t V, const int64_t* faces, const int32_t* offsets, int32_t* cursor,
                                        int32_t* lists, ia_stream_t stream)
{
    IA_REQUIRE(mesh_ok(T, V), "V and 3 * T must fit 31 bits");
    if (T == 0 || V == 0) return IA_OK;
    IA_REQUIRE(faces && offsets && cursor && lists, "null pointer");
    hipError_t e = hipMemsetAsync(cursor, 0, (size_t)V * sizeof(int32_t), (hipStream_t)stream);
    if (e != hipSuccess) {
        ia::set_error("ia_mesh_vertex_faces_fill: %s", hipGetErrorString(e));
        return IA_ERR_LAUNCH;
    }
    vertex_faces_fill_kernel<<<ia::cdiv(T, 256), 256, 0, (hipStream_t)stream>>>(T, V, faces, offsets, cursor, lists);
    return ia::check_launch("ia_mesh_vertex_faces_fill");
}

IA_EXPORT int ia_mesh_vertex_normals(int64_t V, int64_t T, const float* v_pos, const int64_t* faces, const int32_t* offsets,
                                     int32_t* lists, float* v_nrm, ia_stream_t stream)
{
    IA_REQUIRE(mesh_ok(T, V), "V and 3 * T must fit 31 bits");
    if (V == 0) return IA_OK;
    IA_REQUIRE(v_pos && offsets && v_nrm && ((faces && lists) || T == 0), "null pointer");
    vertex_normals_kernel<<<ia::cdiv(V, 256), 256, 0, (hipStream_t)stream>>>(V, T, v_pos, faces, offsets, lists, v_nrm);
    return ia::check_launch("ia_mesh_vertex_normals");
}
