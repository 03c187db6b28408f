// skinning.hip -- building the deformer's skinning-weight grid from a body surface (ForwardDeformer.switch_to_explicit(use_smpl=True) +
// query_weights_smpl, models/deformers/fast_snarf/deformer_torch.py:139-253): voxel centres, brute-force K nearest surface vertices
// (pytorch3d knn_points), inverse-distance blend of the vertices' skinning rows, Jacobi smoothing sweeps.
//
// knn_kernel: one query per lane, 256 per workgroup.  The lane's K-entry list lives in LDS, laid out [k][lane] (a lane's slot k is
// one bank-conflict-free dword column; a dynamically indexed register array would go to scratch); the current last entry
// (d2, index, slot) stays in registers.  Vertices are scanned in ascending index: the first K fill the list, the rest come through
// LDS in tiles of 512 (float4, read as a broadcast).  A vertex replaces the last entry only when its d2 is smaller (its index is
// larger than every index in the list, so an equal d2 never precedes), then a K-slot rescan finds the new last entry.  A per-lane
// selection sort in LDS orders the list, and the workgroup writes its [256, K] block of the outputs with consecutive lanes on
// consecutive addresses.  Nothing depends on P, the tile size or the launch shape: every lane sees every vertex in index order.
// The arithmetic lives in skin_math.h (replayed on the host by tests/skin_harness.c).  Built with -ffp-contract=off.
#include "ia_common.h"
#include "skin_math.h"

namespace {

constexpr int KNN_WG = 256;
constexpr int KNN_TILE = 512;

__global__ __launch_bounds__(KNN_WG) void knn_kernel(int64_t P, int V, int K, const float* __restrict__ p1, const float* __restrict__ p2,
                                                      float* __restrict__ d2_out, int32_t* __restrict__ idx_out)
{
    __shared__ float ld[IA_KNN_MAX_K * KNN_WG];
    __shared__ int32_t li[IA_KNN_MAX_K * KNN_WG];
    __shared__ float4 tile[KNN_TILE];
    const int lane = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * KNN_WG;
    const int64_t p = base + lane < P ? base + lane : P - 1;       // lanes past the end repeat the last query and write nothing
    const float px = p1[3 * p], py = p1[3 * p + 1], pz = p1[3 * p + 2];
    float* md = ld + lane;
    int32_t* mi = li + lane;
    for (int k = 0; k < K; k++) {
        md[k * KNN_WG] = ia_knn_d2(px, py, pz, p2[3 * k], p2[3 * k + 1], p2[3 * k + 2]);
        mi[k * KNN_WG] = k;
    }
    float wd;
    int32_t wi;
    int ws;
    ia_knn_rescan(md, mi, KNN_WG, K, &wd, &wi, &ws);
    for (int v0 = K; v0 < V; v0 += KNN_TILE) {
        __syncthreads();
        for (int t = lane; t < KNN_TILE; t += KNN_WG) {
            const int v = v0 + t;
            // past the last vertex: infinitely far away, d2 = +inf is smaller than nothing
            tile[t] = v < V ? make_float4(p2[3 * (int64_t)v], p2[3 * (int64_t)v + 1], p2[3 * (int64_t)v + 2], 0.f)
                            : make_float4(INFINITY, INFINITY, INFINITY, 0.f);
        }
        __syncthreads();
        const int n = V - v0 < KNN_TILE ? ((V - v0 + 3) & ~3) : KNN_TILE;
        for (int j = 0; j < n; j += 4) {
            float d[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const float4 q = tile[j + u];
                d[u] = ia_knn_d2(px, py, pz, q.x, q.y, q.z);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (d[u] < wd) {
                    md[ws * KNN_WG] = d[u];
                    mi[ws * KNN_WG] = v0 + j + u;
                    ia_knn_rescan(md, mi, KNN_WG, K, &wd, &wi, &ws);
                }
            }
        }
    }
    ia_knn_sort(md, mi, KNN_WG, K, wd, wi, ws);
    __syncthreads();
    const int64_t left = P - base;
    const int total = (int)(left < KNN_WG ? left : KNN_WG) * K;
    for (int f = lane; f < total; f += KNN_WG) {
        const int q = f / K, k = f - q * K;
        d2_out[base * K + f] = ld[k * KNN_WG + q];
        idx_out[base * K + f] = li[k * KNN_WG + q];
    }
}

__global__ __launch_bounds__(256) void skin_blend_kernel(int64_t P, int V, int K, const float* __restrict__ d2, const int32_t* __restrict__ idx,
                                                          const float* __restrict__ weights, float* __restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int32_t* row = idx + p * K;
    bool ok = true;
    for (int k = 0; k < K; k++) ok = ok && (uint32_t)row[k] < (uint32_t)V;
    if (!ok) {                                                      // an index outside the vertex table: no read, the row is NaN
        for (int c = 0; c < IA_SKIN_CHANNELS; c++) out[c * P + p] = NAN;
        return;
    }
    ia_skin_blend_row(d2 + p * K, row, K, weights, out + p, P);
}

__global__ __launch_bounds__(256) void skin_smooth_kernel(int D, int H, int W, const float* __restrict__ src, float* __restrict__ dst)
{
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= (int64_t)D * H * W) return;
    const int w = (int)(v % W), h = (int)((v / W) % H), d = (int)(v / ((int64_t)W * H));
    ia_skin_smooth_voxel(src, dst, d, h, w, D, H, W);
}

__global__ __launch_bounds__(256) void skin_grid_points_kernel(int D, int H, int W, float ratio, float scale, float ox, float oy, float oz,
                                                                float* __restrict__ out)
{
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= (int64_t)D * H * W) return;
    const int w = (int)(v % W), h = (int)((v / W) % H), d = (int)(v / ((int64_t)W * H));
    const float offset[3] = {ox, oy, oz};
    float r[3];
    ia_skin_grid_point(d, h, w, D, H, W, ratio, scale, offset, r);
    out[3 * v] = r[0];
    out[3 * v + 1] = r[1];
    out[3 * v + 2] = r[2];
}

bool grid_ok(int D, int H, int W) { return D >= 1 && H >= 1 && W >= 1 && (int64_t)D * H * W * IA_SKIN_CHANNELS <= INT32_MAX; }

}  // namespace

IA_EXPORT int ia_knn_points(int64_t P, int V, int K, const float* p1, const float* p2, float* d2, int32_t* idx, ia_stream_t stream)
{
    IA_REQUIRE(K >= 1 && K <= IA_KNN_MAX_K, "K must be in 1 .. 32");
    IA_REQUIRE(V >= K, "fewer than K points in p2");
    IA_REQUIRE(P >= 0, "negative query count");
    if (P == 0) return IA_OK;
    IA_REQUIRE(p1 && p2 && d2 && idx, "null pointer");
    knn_kernel<<<ia::cdiv(P, KNN_WG), KNN_WG, 0, (hipStream_t)stream>>>(P, V, K, p1, p2, d2, idx);
    return ia::check_launch("ia_knn_points");
}

IA_EXPORT int ia_skin_blend(int64_t P, int V, int K, const float* d2, const int32_t* idx, const float* weights, float* out,
                            ia_stream_t stream)
{
    IA_REQUIRE(K >= 1 && K <= IA_KNN_MAX_K, "K must be in 1 .. 32");
    IA_REQUIRE(V >= 1 && P >= 0, "empty vertex table or negative query count");
    if (P == 0) return IA_OK;
    IA_REQUIRE(d2 && idx && weights && out, "null pointer");
    skin_blend_kernel<<<ia::cdiv(P, 256), 256, 0, (hipStream_t)stream>>>(P, V, K, d2, idx, weights, out);
    return ia::check_launch("ia_skin_blend");
}

IA_EXPORT int ia_skin_smooth(int D, int H, int W, const float* src, float* dst, ia_stream_t stream)
{
    IA_REQUIRE(grid_ok(D, H, W), "grid sides must be >= 1 and 24 * D * H * W must fit 31 bits");
    IA_REQUIRE(src && dst && src != dst, "null pointer, or src == dst (a sweep reads the old buffer: ping-pong two)");
    skin_smooth_kernel<<<ia::cdiv((int64_t)D * H * W, 256), 256, 0, (hipStream_t)stream>>>(D, H, W, src, dst);
    return ia::check_launch("ia_skin_smooth");
}

IA_EXPORT int ia_skin_grid_points(int D, int H, int W, float ratio, float scale, float ox, float oy, float oz, float* out,
                                  ia_stream_t stream)
{
    IA_REQUIRE(grid_ok(D, H, W), "grid sides must be >= 1 and 24 * D * H * W must fit 31 bits");
    IA_REQUIRE(out, "null pointer");
    skin_grid_points_kernel<<<ia::cdiv((int64_t)D * H * W, 256), 256, 0, (hipStream_t)stream>>>(D, H, W, ratio, scale, ox, oy, oz, out);
    return ia::check_launch("ia_skin_grid_points");
}
