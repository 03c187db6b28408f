// mcubes.hip -- canonical mesh export: dense marching cubes of a level grid (models/rf/geometry.py:14-104, MarchingCubeHelper ->
// mcubes.marching_cubes(-level, threshold)) and the grid points of BaseImplicitGeometry.isosurface_ that feed it.
//
// Grid points are handed out in C order, one per lane, 256 per workgroup; a point's lane also owns the cell whose lowest corner it is.
// Three passes over the level grid, each recomputing the per-point work from the grid (no per-cell scratch):
//   count  owned crossed edges (vertices) and triangles per point -> per-workgroup totals; two ia_exclusive_scan_i64 turn them into
//          workgroup bases and the grand totals (the caller's one read-back sizes the outputs)
//   emit   ranks the vertices inside the workgroup (ballot bit-planes + mbcnt), writes the scaled vertex positions and the point's
//          first vertex id [nx*ny*nz] int32
//   face   ranks the triangles the same way; each triangle edge -> owning point's first id + rank of the axis among that point's
//          crossed owned edges; int64 faces in cell order then table order
// The arithmetic lives in mc_math.h (replayed on the host by tests/mc_harness.c).  Built with -ffp-contract=off.
#include "ia_common.h"
#include "mc_math.h"

namespace {

constexpr int MC_THREADS = 256;

struct Dims {
    int nx, ny, nz;
    uint32_t syz, n;
};

__device__ __forceinline__ void coords(const Dims& d, uint32_t p, int& i, int& j, int& k)
{
    i = (int)(p / d.syz);
    const uint32_t r = p - (uint32_t)i * d.syz;
    j = (int)(r / (uint32_t)d.nz);
    k = (int)(r - (uint32_t)j * (uint32_t)d.nz);
}

// owned-edge mask of point p and (when p is the lowest corner of a cell) the cell's cube index (-1: no cell)
__device__ __forceinline__ void point_work(const float* __restrict__ L, const Dims& d, uint32_t p, float thr, int& mask, int& cube)
{
    int i, j, k;
    coords(d, p, i, j, k);
    const int hx = i + 1 < d.nx, hy = j + 1 < d.ny, hz = k + 1 < d.nz;
    const float l0 = L[p];
    const float lx = hx ? L[p + d.syz] : 0.f, ly = hy ? L[p + d.nz] : 0.f, lz = hz ? L[p + 1] : 0.f;
    mask = ia_mc_owned_mask(l0, lx, ly, lz, hx, hy, hz, thr);
    cube = -1;
    if (hx && hy && hz) {
        const float c[8] = {l0, lx, L[p + d.syz + d.nz], ly, lz, L[p + d.syz + 1], L[p + d.syz + d.nz + 1], L[p + d.nz + 1]};
        cube = ia_mc_cube_index(c, thr);
    }
}

__device__ __forceinline__ int lane_prefix(uint64_t m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// exclusive prefix of a small count c (< 2^BITS) over the workgroup, by ballot bit-planes; total of the workgroup in *total
template <int BITS>
__device__ __forceinline__ int block_prefix(int c, int* wave_tot /*LDS [MC_THREADS / 64]*/, int* total)
{
    const int wid = threadIdx.x >> 6;
    int pre = 0, wsum = 0;
#pragma unroll
    for (int b = 0; b < BITS; b++) {
        const uint64_t m = __ballot((c >> b) & 1);
        pre += lane_prefix(m) << b;
        wsum += __popcll(m) << b;
    }
    if ((threadIdx.x & 63) == 0) wave_tot[wid] = wsum;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < MC_THREADS / 64; w++) {
        const int t = wave_tot[w];
        off += w < wid ? t : 0;
        tot += t;
    }
    *total = tot;
    return off + pre;
}

__global__ __launch_bounds__(MC_THREADS) void mc_count_kernel(const float* __restrict__ L, Dims d, float thr, int64_t* __restrict__ vcnt,
                                                               int64_t* __restrict__ tcnt)
{
    __shared__ int wv[MC_THREADS / 64], wt[MC_THREADS / 64];
    const uint32_t p = blockIdx.x * MC_THREADS + threadIdx.x;
    int nv = 0, nt = 0;
    if (p < d.n) {
        int mask, cube;
        point_work(L, d, p, thr, mask, cube);
        nv = __popc(mask);
        nt = cube >= 0 ? ia_mc_n_tri(cube) : 0;
    }
    int tv, tt;
    block_prefix<2>(nv, wv, &tv);
    block_prefix<3>(nt, wt, &tt);
    if (threadIdx.x == 0) {
        vcnt[blockIdx.x] = tv;
        tcnt[blockIdx.x] = tt;
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_emit_kernel(const float* __restrict__ L, Dims d, float thr, const int64_t* __restrict__ vstart,
                                                              float bx0, float by0, float bz0, float bx1, float by1, float bz1,
                                                              int32_t* __restrict__ first_vid, float* __restrict__ v_pos)
{
    __shared__ int wv[MC_THREADS / 64];
    const uint32_t p = blockIdx.x * MC_THREADS + threadIdx.x;
    int mask = 0, cube;
    if (p < d.n) point_work(L, d, p, thr, mask, cube);
    int tot;
    const int pre = block_prefix<2>(__popc(mask), wv, &tot);
    if (p >= d.n) return;
    const int64_t id = vstart[blockIdx.x] + pre;
    first_vid[p] = (int32_t)id;
    if (!mask) return;
    int i, j, k;
    coords(d, p, i, j, k);
    const float l0 = L[p];
    const float lo[3] = {bx0, by0, bz0}, hi[3] = {bx1, by1, bz1};
    const int idx[3] = {i, j, k}, n[3] = {d.nx, d.ny, d.nz};
    const uint32_t stride[3] = {d.syz, (uint32_t)d.nz, 1u};
    int64_t v = id;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (!(mask >> a & 1)) continue;
        const float ca = ia_mc_edge_coord(idx[a], l0, L[p + stride[a]], thr);
#pragma unroll
        for (int c = 0; c < 3; c++) v_pos[3 * v + c] = ia_mc_scale(c == a ? ca : (float)idx[c], n[c], lo[c], hi[c]);
        v++;
    }
}

// rank of the axis-a vertex of point q = (qi, qj, qk) among q's crossed owned edges (only x and y can precede)
__device__ __forceinline__ int axis_rank(const float* __restrict__ L, const Dims& d, uint32_t q, int qi, int qj, int axis, float thr)
{
    if (axis == 0) return 0;
    const int in0 = ia_mc_inside(L[q], thr);
    int r = (qi + 1 < d.nx && ia_mc_inside(L[q + d.syz], thr) != in0) ? 1 : 0;
    if (axis == 2) r += (qj + 1 < d.ny && ia_mc_inside(L[q + d.nz], thr) != in0) ? 1 : 0;
    return r;
}

__global__ __launch_bounds__(MC_THREADS) void mc_face_kernel(const float* __restrict__ L, Dims d, float thr, const int64_t* __restrict__ tstart,
                                                              const int32_t* __restrict__ first_vid, int64_t* __restrict__ faces)
{
    __shared__ int wt[MC_THREADS / 64];
    const uint32_t p = blockIdx.x * MC_THREADS + threadIdx.x;
    int mask, cube = -1;
    if (p < d.n) point_work(L, d, p, thr, mask, cube);
    const int nt = cube >= 0 ? ia_mc_n_tri(cube) : 0;
    int tot;
    const int pre = block_prefix<3>(nt, wt, &tot);
    if (nt == 0) return;
    int i, j, k;
    coords(d, p, i, j, k);
    int64_t f = tstart[blockIdx.x] + pre;
    for (int t = 0; t < nt; t++, f++) {
        int64_t id[3];
#pragma unroll
        for (int e = 0; e < 3; e++) {
            const int edge = ia_mc_tri_table[cube][3 * t + e];
            const int o = ia_mc_corner_xyz[ia_mc_edge_owner[edge]];
            const int qi = i + (o & 1), qj = j + ((o >> 1) & 1);
            const uint32_t q = p + ((o & 1) ? d.syz : 0u) + ((o & 2) ? (uint32_t)d.nz : 0u) + ((o & 4) ? 1u : 0u);
            id[e] = (int64_t)first_vid[q] + axis_rank(L, d, q, qi, qj, ia_mc_edge_axis[edge], thr);
        }
        faces[3 * f + 0] = id[0];
        faces[3 * f + 1] = id[IA_MC_FLIP ? 2 : 1];
        faces[3 * f + 2] = id[IA_MC_FLIP ? 1 : 2];
    }
}

// normalized hash-grid coordinates of grid points [start, start + n): ((axis value) - center) / scale + 0.5, as ia_normalize_points
__global__ __launch_bounds__(256) void mc_grid_points_kernel(int64_t n, uint32_t start, Dims d, const float* __restrict__ axes,
                                                              const float* __restrict__ center, const float* __restrict__ scale,
                                                              float* __restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    int i, j, k;
    coords(d, start + (uint32_t)t, i, j, k);
    const float a[3] = {axes[i], axes[d.nx + j], axes[d.nx + d.ny + k]};
#pragma unroll
    for (int c = 0; c < 3; c++) out[3 * t + c] = (a[c] - center[c]) / scale[c] + 0.5f;
}

int64_t n_blocks(int64_t n) { return (n + MC_THREADS - 1) / MC_THREADS; }

struct Scratch {
    int64_t *vcnt, *tcnt, *vstart, *tstart;
    void* scan_tmp;
};

// per-block vertex / triangle counts, their exclusive scans, the scan work area; scratch 8-byte aligned
size_t mc_layout(void* scratch, int64_t blocks, Scratch* sc)
{
    ia::Carver c(scratch);
    sc->vcnt = c.take<int64_t>((size_t)blocks, 8);
    sc->tcnt = c.take<int64_t>((size_t)blocks, 8);
    sc->vstart = c.take<int64_t>((size_t)blocks, 8);
    sc->tstart = c.take<int64_t>((size_t)blocks, 8);
    sc->scan_tmp = c.take<char>((size_t)ia_scan_tmp_bytes(blocks), 8);
    return c.need(8);
}

bool dims_ok(int nx, int ny, int nz, Dims* d)
{
    if (nx < 2 || ny < 2 || nz < 2) return false;
    const int64_t n = (int64_t)nx * ny * nz;
    if (n > INT32_MAX) return false;
    *d = Dims{nx, ny, nz, (uint32_t)((int64_t)ny * nz), (uint32_t)n};
    return true;
}

}  // namespace

IA_EXPORT int64_t ia_mc_scratch_bytes(int nx, int ny, int nz)
{
    const int64_t blocks = n_blocks((int64_t)(nx > 0 ? nx : 0) * (ny > 0 ? ny : 0) * (nz > 0 ? nz : 0));
    Scratch sc;
    return (int64_t)mc_layout(nullptr, blocks, &sc);
}

IA_EXPORT int ia_mc_count(int nx, int ny, int nz, const float* level, float threshold, void* scratch, int64_t* totals,
                          ia_stream_t stream)
{
    Dims d;
    IA_REQUIRE(dims_ok(nx, ny, nz, &d), "grid must be at least 2 x 2 x 2 and hold fewer than 2^31 points");
    IA_REQUIRE(level && scratch && totals, "null pointer");
    const hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = n_blocks(d.n);
    Scratch sc;
    mc_layout(scratch, blocks, &sc);
    mc_count_kernel<<<(unsigned)blocks, MC_THREADS, 0, s>>>(level, d, threshold, sc.vcnt, sc.tcnt);
    int r = ia::check_launch("ia_mc_count");
    if (r != IA_OK) return r;
    r = ia_exclusive_scan_i64(sc.vcnt, sc.vstart, totals, blocks, sc.scan_tmp, stream);
    if (r != IA_OK) return r;
    return ia_exclusive_scan_i64(sc.tcnt, sc.tstart, totals + 1, blocks, sc.scan_tmp, stream);
}

IA_EXPORT int ia_mc_emit(int nx, int ny, int nz, const float* level, float threshold, const float* box, const void* scratch,
                         int32_t* first_vid, float* v_pos, int64_t* t_pos_idx, ia_stream_t stream)
{
    Dims d;
    IA_REQUIRE(dims_ok(nx, ny, nz, &d), "grid must be at least 2 x 2 x 2 and hold fewer than 2^31 points");
    IA_REQUIRE(level && box && scratch && first_vid && v_pos && t_pos_idx, "null pointer");
    const hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = n_blocks(d.n);
    Scratch sc;
    mc_layout((void*)scratch, blocks, &sc);
    mc_emit_kernel<<<(unsigned)blocks, MC_THREADS, 0, s>>>(level, d, threshold, sc.vstart, box[0], box[1], box[2], box[3], box[4], box[5],
                                                          first_vid, v_pos);
    mc_face_kernel<<<(unsigned)blocks, MC_THREADS, 0, s>>>(level, d, threshold, sc.tstart, first_vid, t_pos_idx);
    return ia::check_launch("ia_mc_emit");
}

IA_EXPORT int ia_mc_grid_points(int64_t n, int64_t start, int nx, int ny, int nz, const float* axes, const float* center,
                                const float* scale, float* out, ia_stream_t stream)
{
    Dims d;
    IA_REQUIRE(dims_ok(nx, ny, nz, &d), "grid must be at least 2 x 2 x 2 and hold fewer than 2^31 points");
    IA_REQUIRE(start >= 0 && n >= 0 && start + n <= (int64_t)d.n, "point range outside the grid");
    if (n == 0) return IA_OK;
    IA_REQUIRE(axes && center && scale && out, "null pointer");
    mc_grid_points_kernel<<<ia::cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(n, (uint32_t)start, d, axes, center, scale, out);
    return ia::check_launch("ia_mc_grid_points");
}
