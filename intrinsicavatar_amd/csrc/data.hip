// data.hip -- training batches on the device: camera rays, the samplers' edge band and index lists, and the per-step batch kernel
// (datasets/peoplesnapshot.py:19-33 and :119-175, utils/sampler.py:9-67).
//
//   window   one workgroup owns a tile of TL positions along the window axis x TI positions along the inner axis, stages the tile plus a
//            halo of k - 1 positions in LDS, and each lane forms the windows of its elements from LDS; minimum and maximum leave in one pass.
//            <256, 1> serves a contiguous axis (the flat mask, image rows), <64, 64> a strided one (image columns: lanes run along the rows).
//   lists    count -> ia_exclusive_scan_i32 -> fill over workgroups of 256 pixels that never straddle a frame; ranks inside a workgroup by
//            ballot + mbcnt, so both lists come out ascending.
//   sample   one row per lane: draw -> pixel -> mask value, colour, ray, near / far.  The list sizes are read from the CSR offsets on the
//            device; an empty list that rows were asked from sets the status word.
//   truth    ground-truth frames (datasets/rana.py, synthetichuman.py): one workgroup per frame bounds the mask and writes the valid
//            rectangle (integer minima in the wave, then through LDS); one row per lane gathers albedo / normal / valid at the pixels
//            ia_sample_batch chose; one lane per output element takes the centre 2 x 2 of an even integer downscale.
// The arithmetic lives in data_math.h (replayed on the host by tests/data_harness.c and tests/truth_harness.c).  Built with -ffp-contract=off.
#include "ia_common.h"
#include "data_math.h"

namespace {

constexpr int DT = 256;

struct Cam {
    double v[21];
};

__global__ __launch_bounds__(DT) void make_rays_kernel(int64_t n, const int64_t* __restrict__ pixels, int64_t n_pixels, int W, Cam cam,
                                                        float* __restrict__ rays_o, float* __restrict__ rays_d)
{
    const int64_t j = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (j >= n) return;
    const int64_t p = pixels ? pixels[j] : j;
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
    if (p >= 0 && p < n_pixels) ia_data_ray(p, W, cam.v, o, d);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        rays_o[3 * j + c] = o[c];
        rays_d[3 * j + c] = d[c];
    }
}

template <int TL, int TI>
__global__ __launch_bounds__(DT) void window_kernel(int64_t len, int64_t inner, int k, int64_t tiles_l, int64_t tiles_i,
                                                     const float* __restrict__ in, float* __restrict__ out_min, float* __restrict__ out_max)
{
    __shared__ float tile[(TL + IA_WINDOW_MAX_K - 1) * TI];
    int64_t b = blockIdx.x;
    const int64_t ti = b % tiles_i;
    b /= tiles_i;
    const int64_t tl = b % tiles_l, o = b / tiles_l;
    const int64_t l0 = tl * TL, i0 = ti * TI;
    const int64_t h0 = l0 - k / 2;                       // position of LDS row 0 along the window axis
    const int rows = TL + k - 1;
    const int64_t base = o * len * inner;
    for (int e = threadIdx.x; e < rows * TI; e += DT) {
        const int64_t l = h0 + e / TI, i = i0 + e % TI;
        tile[e] = (l >= 0 && l < len && i < inner) ? in[base + l * inner + i] : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < TL * TI; e += DT) {
        const int c = e % TI;
        const int64_t l = l0 + e / TI, i = i0 + c;
        if (l >= len || i >= inner) continue;
        int64_t lo, hi;
        ia_data_window_range(l, len, k, &lo, &hi);       // h0 <= lo < hi <= h0 + rows
        float mn, mx;
        ia_data_minmax(tile + c, lo - h0, hi - h0, TI, &mn, &mx);
        if (out_min) out_min[base + l * inner + i] = mn;
        if (out_max) out_max[base + l * inner + i] = mx;
    }
}

__device__ __forceinline__ int lane_prefix(uint64_t m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// exclusive rank of a flag over the workgroup (ballot + mbcnt inside a wave, wave totals through LDS); the workgroup's total in *total
__device__ __forceinline__ int flag_rank(int flag, int* wave_tot /*LDS [DT / 64]*/, int* total)
{
    const int wid = threadIdx.x >> 6;
    const uint64_t m = __ballot(flag);
    if ((threadIdx.x & 63) == 0) wave_tot[wid] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < DT / 64; w++) {
        const int t = wave_tot[w];
        off += w < wid ? t : 0;
        tot += t;
    }
    *total = tot;
    return off + lane_prefix(m);
}

struct Lists {
    int32_t *mcnt, *ecnt, *mstart, *estart;
    void* scan_tmp;
};

__device__ __forceinline__ void pixel_flags(const float* __restrict__ mask, const float* __restrict__ mask_i, const float* __restrict__ mask_o,
                                            int64_t bpf, int64_t N, int64_t* f, int64_t* p, int* m, int* e)
{
    *f = blockIdx.x / bpf;
    *p = (blockIdx.x % bpf) * DT + threadIdx.x;
    *m = 0;
    *e = 0;
    if (*p < N) {
        const int64_t g = *f * N + *p;
        *m = mask[g] != 0.0f;
        *e = ia_data_is_edge(mask_i[g], mask_o[g]);
    }
}

__global__ __launch_bounds__(DT) void lists_count_kernel(int64_t bpf, int64_t N, const float* __restrict__ mask, const float* __restrict__ mask_i,
                                                          const float* __restrict__ mask_o, int32_t* __restrict__ mcnt, int32_t* __restrict__ ecnt)
{
    __shared__ int wm[DT / 64], we[DT / 64];
    int64_t f, p;
    int m, e, tm, te;
    pixel_flags(mask, mask_i, mask_o, bpf, N, &f, &p, &m, &e);
    flag_rank(m, wm, &tm);
    flag_rank(e, we, &te);
    if (threadIdx.x == 0) {
        mcnt[blockIdx.x] = tm;
        ecnt[blockIdx.x] = te;
    }
}

__global__ __launch_bounds__(DT) void lists_fill_kernel(int64_t F, int64_t bpf, int64_t N, const float* __restrict__ mask,
                                                         const float* __restrict__ mask_i, const float* __restrict__ mask_o,
                                                         const int32_t* __restrict__ mstart, const int32_t* __restrict__ estart,
                                                         const int32_t* __restrict__ totals, int32_t* __restrict__ mask_start,
                                                         int32_t* __restrict__ edge_start, int32_t* __restrict__ counts,
                                                         int32_t* __restrict__ mask_loc, int32_t* __restrict__ edge_loc)
{
    __shared__ int wm[DT / 64], we[DT / 64];
    int64_t f, p;
    int m, e, tm, te;
    pixel_flags(mask, mask_i, mask_o, bpf, N, &f, &p, &m, &e);
    const int rm = flag_rank(m, wm, &tm), re = flag_rank(e, we, &te);
    const int32_t bm = mstart[blockIdx.x], be = estart[blockIdx.x];
    if (m) mask_loc[bm + rm] = (int32_t)p;
    if (e) edge_loc[be + re] = (int32_t)p;
    if (threadIdx.x == 0 && blockIdx.x % bpf == 0) {     // the frame's first workgroup: its CSR offsets and sizes
        const int32_t nm = f + 1 < F ? mstart[blockIdx.x + bpf] : totals[0], ne = f + 1 < F ? estart[blockIdx.x + bpf] : totals[1];
        mask_start[f] = bm;
        edge_start[f] = be;
        counts[2 * f] = nm - bm;
        counts[2 * f + 1] = ne - be;
        if (f + 1 == F) {
            mask_start[F] = totals[0];
            edge_start[F] = totals[1];
        }
    }
}

__global__ __launch_bounds__(DT) void sample_kernel(int64_t n, int64_t num_mask, int64_t num_edge, int64_t frame, int64_t N, int W,
                                                     const int64_t* __restrict__ words, const float* __restrict__ masks,
                                                     const uint8_t* __restrict__ images, const int32_t* __restrict__ mask_start,
                                                     const int32_t* __restrict__ edge_start, const int32_t* __restrict__ mask_loc,
                                                     const int32_t* __restrict__ edge_loc, Cam cam, const float* __restrict__ near_tab,
                                                     const float* __restrict__ far_tab, int64_t* __restrict__ indices, float* __restrict__ alpha,
                                                     float* __restrict__ rgb, float* __restrict__ rays_o, float* __restrict__ rays_d,
                                                     float* __restrict__ near, float* __restrict__ far, int32_t* __restrict__ status)
{
    const int64_t j = (int64_t)blockIdx.x * DT + threadIdx.x;
    const int32_t m0 = num_mask > 0 ? mask_start[frame] : 0, n_mask = num_mask > 0 ? mask_start[frame + 1] - m0 : 0;
    const int32_t e0 = num_edge > 0 ? edge_start[frame] : 0, n_edge = num_edge > 0 ? edge_start[frame + 1] - e0 : 0;
    if (j == 0) *status = ((num_mask > 0 && n_mask <= 0) ? 1 : 0) | ((num_edge > 0 && n_edge <= 0) ? 2 : 0);
    if (j >= n) return;
    const int64_t w = words ? (words[j] & INT64_MAX) : j;      // words are non-negative by contract; the sign bit can not leave the lists
    int64_t p = -1;
    if (j < num_mask) {
        if (n_mask > 0) p = mask_loc[m0 + ia_data_pick(w, n_mask)];
    } else if (j < num_mask + num_edge) {
        if (n_edge > 0) p = edge_loc[e0 + ia_data_pick(w, n_edge)];
    } else {
        p = ia_data_pick(w, N);
    }
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f}, c[3] = {0.f, 0.f, 0.f}, a = 0.f, tn = 0.f, tf = 0.f;
    if (p >= 0 && p < N) {
        const int64_t g = frame * N + p;
        a = masks[g];
#pragma unroll
        for (int k = 0; k < 3; k++) c[k] = ia_data_u8(images[3 * g + k]);
        ia_data_ray(p, W, cam.v, o, d);
        tn = near_tab[frame];
        tf = far_tab[frame];
    } else {
        p = -1;
    }
    indices[j] = p;
    alpha[j] = a;
    near[j] = tn;
    far[j] = tf;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        rgb[3 * j + k] = c[k];
        rays_o[3 * j + k] = o[k];
        rays_d[3 * j + k] = d[k];
    }
}

// ---- ground-truth frames (datasets/rana.py, datasets/synthetichuman.py): the valid rectangle, the albedo / normal / valid rows, the downscale
__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

// one workgroup per frame: integer bounds of the pixels that count, reduced in the wave, then over the four waves through LDS
__global__ __launch_bounds__(DT) void valid_rect_kernel(int H, int W, int k, const float* __restrict__ masks, int32_t* __restrict__ rect)
{
    __shared__ int part[DT / 64][4];
    const int64_t N = (int64_t)H * W, f = blockIdx.x;
    const float* __restrict__ m = masks + f * N;
    // (xmin, ymin, -xmax, -ymax): four minima; the empty set is (W, H, 1, 1), i.e. xmax = ymax = -1
    int b[4] = {W, H, 1, 1};
    for (int64_t p = threadIdx.x; p < N; p += DT) {
        if (!ia_data_mask_counts(m[p])) continue;
        const int x = (int)(p % W), y = (int)(p / W);
        b[0] = x < b[0] ? x : b[0];
        b[1] = y < b[1] ? y : b[1];
        b[2] = -x < b[2] ? -x : b[2];
        b[3] = -y < b[3] ? -y : b[3];
    }
#pragma unroll
    for (int c = 0; c < 4; c++) b[c] = wave_min(b[c]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 4; c++) part[threadIdx.x >> 6][c] = b[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < DT / 64; w++)
#pragma unroll
            for (int c = 0; c < 4; c++) b[c] = part[w][c] < b[c] ? part[w][c] : b[c];
        int32_t r[4];
        ia_data_valid_rect(b[0], b[1], -b[2], -b[3], H, W, k, r);
#pragma unroll
        for (int c = 0; c < 4; c++) rect[4 * f + c] = r[c];
    }
}

__global__ __launch_bounds__(DT) void sample_truth_kernel(int64_t n, int64_t frame, int64_t N, int W, const int64_t* __restrict__ pixels,
                                                           const uint8_t* __restrict__ albedos, const uint8_t* __restrict__ normals,
                                                           const int32_t* __restrict__ rect, float* __restrict__ albedo,
                                                           float* __restrict__ normal, uint8_t* __restrict__ valid)
{
    const int64_t j = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (j >= n) return;
    const int64_t p = pixels ? pixels[j] : j;
    float a[3] = {0.f, 0.f, 0.f}, nr[3] = {0.f, 0.f, 0.f};
    uint8_t v = 0;
    if (p >= 0 && p < N) {
        const int64_t g = frame * N + p;
        int32_t r[4];
#pragma unroll
        for (int c = 0; c < 4; c++) r[c] = rect[4 * frame + c];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            a[c] = ia_data_u8(albedos[3 * g + c]);
            nr[c] = ia_data_normal_u8(normals[3 * g + c]);
        }
        v = (uint8_t)ia_data_in_rect(p, W, r);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        albedo[3 * j + c] = a[c];
        normal[3 * j + c] = nr[c];
    }
    valid[j] = v;
}

// in [F,H,W,C] -> out [F,Ho,Wo,C], one lane per output element (C = 1: a plain [F,H,W] array)
template <typename T>
__global__ __launch_bounds__(DT) void downscale_center_kernel(int64_t total, int H, int W, int C, int s, const T* __restrict__ in,
                                                               T* __restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (e >= total) return;
    const int Ho = H / s, Wo = W / s;
    int64_t t = e;
    const int c = (int)(t % C);
    t /= C;
    const int64_t xo = t % Wo;
    t /= Wo;
    const int64_t yo = t % Ho, f = t / Ho;
    const int64_t x0 = ia_data_center_src(xo, s), y0 = ia_data_center_src(yo, s);      // 0 <= x0, x0 + 1 < W; the same in y (s even, W % s == 0)
    const int64_t at = ((f * H + y0) * W + x0) * C + c, row = (int64_t)W * C;
    if constexpr (sizeof(T) == 1)
        out[e] = ia_data_center_u8(in[at], in[at + C], in[at + row], in[at + row + C]);
    else
        out[e] = ia_data_center_f32(in[at], in[at + C], in[at + row], in[at + row + C]);
}

template <typename T>
int downscale_center(const char* what, int64_t F, int H, int W, int C, int s, const T* in, T* out, ia_stream_t stream)
{
    IA_REQUIRE(F >= 0 && H > 0 && W > 0 && C >= 1, "bad extent");
    IA_REQUIRE(s >= 2 && s % 2 == 0 && H % s == 0 && W % s == 0, "the centre rule needs an even factor that divides both sides");
    const int64_t per = (int64_t)(H / s) * (W / s) * C;
    IA_REQUIRE(F == 0 || per <= INT64_MAX / 4 / F, "too many elements");
    const int64_t total = F * per;
    if (total == 0) return IA_OK;
    IA_REQUIRE(in && out && (const void*)in != (const void*)out, "null pointer or in-place call");
    IA_REQUIRE((total + DT - 1) / DT <= INT32_MAX, "too many elements for one launch");
    downscale_center_kernel<T><<<(unsigned)((total + DT - 1) / DT), DT, 0, (hipStream_t)stream>>>(total, H, W, C, s, in, out);
    return ia::check_launch(what);
}

// per-block counts of the two lists, their exclusive scans, the scan work area; scratch 8-byte aligned
size_t lists_layout(void* scratch, int64_t blocks, Lists* L)
{
    ia::Carver c(scratch);
    L->mcnt = c.take<int32_t>((size_t)blocks, 8);
    L->ecnt = c.take<int32_t>((size_t)blocks, 8);
    L->mstart = c.take<int32_t>((size_t)blocks, 8);
    L->estart = c.take<int32_t>((size_t)blocks, 8);
    L->scan_tmp = c.take<char>((size_t)ia_scan_tmp_bytes(blocks), 8);
    return c.need(8);
}

bool lists_dims(int64_t F, int64_t N, int64_t* bpf, int64_t* blocks)
{
    if (F < 1 || N < 1 || N > INT32_MAX || F > INT32_MAX / N) return false;
    *bpf = (N + DT - 1) / DT;
    *blocks = F * *bpf;
    return *blocks <= INT32_MAX;
}

Cam load_cam(const double* cam_host)
{
    Cam c;
    for (int i = 0; i < 21; i++) c.v[i] = cam_host[i];
    return c;
}

}  // namespace

IA_EXPORT int ia_make_rays(int64_t n, const int64_t* pixels, int H, int W, const double* cam_host, float* rays_o, float* rays_d,
                           ia_stream_t stream)
{
    IA_REQUIRE(H > 0 && W > 0 && n >= 0, "bad image size or row count");
    IA_REQUIRE(pixels || n <= (int64_t)H * W, "without a pixel list the rows are the frame's first n pixels");
    if (n == 0) return IA_OK;
    IA_REQUIRE(cam_host && rays_o && rays_d, "null pointer");
    IA_REQUIRE((n + DT - 1) / DT <= INT32_MAX, "too many rows");
    make_rays_kernel<<<ia::cdiv(n, DT), DT, 0, (hipStream_t)stream>>>(n, pixels, (int64_t)H * W, W, load_cam(cam_host), rays_o, rays_d);
    return ia::check_launch("ia_make_rays");
}

IA_EXPORT int ia_window_minmax(int64_t outer, int64_t len, int64_t inner, int k, const float* in, float* out_min, float* out_max,
                               ia_stream_t stream)
{
    IA_REQUIRE(k >= 1 && k <= IA_WINDOW_MAX_K, "window must have 1 to 64 taps");
    IA_REQUIRE(outer >= 0 && len >= 0 && inner >= 0, "negative extent");
    if (outer == 0 || len == 0 || inner == 0) return IA_OK;
    IA_REQUIRE(in && (out_min || out_max), "null pointer");
    IA_REQUIRE(in != out_min && in != out_max, "the window kernel does not work in place");
    const hipStream_t s = (hipStream_t)stream;
    const int TL = inner == 1 ? 256 : 64, TI = inner == 1 ? 1 : 64;
    const int64_t tiles_l = (len + TL - 1) / TL, tiles_i = (inner + TI - 1) / TI;
    IA_REQUIRE(tiles_l <= INT32_MAX / tiles_i && outer <= INT32_MAX / (tiles_l * tiles_i), "too many tiles for one launch");
    const unsigned blocks = (unsigned)(outer * tiles_l * tiles_i);
    if (inner == 1)
        window_kernel<256, 1><<<blocks, DT, 0, s>>>(len, inner, k, tiles_l, tiles_i, in, out_min, out_max);
    else
        window_kernel<64, 64><<<blocks, DT, 0, s>>>(len, inner, k, tiles_l, tiles_i, in, out_min, out_max);
    return ia::check_launch("ia_window_minmax");
}

IA_EXPORT int64_t ia_flag_lists_scratch_bytes(int64_t F, int64_t N)
{
    int64_t bpf, blocks;
    if (!lists_dims(F, N, &bpf, &blocks)) return 0;
    Lists L;
    return (int64_t)lists_layout(nullptr, blocks, &L);
}

IA_EXPORT int ia_flag_lists_count(int64_t F, int64_t N, const float* mask, const float* mask_i, const float* mask_o, void* scratch,
                                  int32_t* totals, ia_stream_t stream)
{
    int64_t bpf, blocks;
    IA_REQUIRE(lists_dims(F, N, &bpf, &blocks), "need F >= 1 frames of N >= 1 pixels with F * N < 2^31");
    IA_REQUIRE(mask && mask_i && mask_o && scratch && totals, "null pointer");
    Lists L;
    lists_layout(scratch, blocks, &L);
    lists_count_kernel<<<(unsigned)blocks, DT, 0, (hipStream_t)stream>>>(bpf, N, mask, mask_i, mask_o, L.mcnt, L.ecnt);
    int r = ia::check_launch("ia_flag_lists_count");
    if (r != IA_OK) return r;
    r = ia_exclusive_scan_i32(L.mcnt, L.mstart, totals, blocks, L.scan_tmp, stream);
    if (r != IA_OK) return r;
    return ia_exclusive_scan_i32(L.ecnt, L.estart, totals + 1, blocks, L.scan_tmp, stream);
}

IA_EXPORT int ia_flag_lists_fill(int64_t F, int64_t N, const float* mask, const float* mask_i, const float* mask_o, const void* scratch,
                                 const int32_t* totals, int32_t* mask_start, int32_t* edge_start, int32_t* counts, int32_t* mask_loc,
                                 int32_t* edge_loc, ia_stream_t stream)
{
    int64_t bpf, blocks;
    IA_REQUIRE(lists_dims(F, N, &bpf, &blocks), "need F >= 1 frames of N >= 1 pixels with F * N < 2^31");
    IA_REQUIRE(mask && mask_i && mask_o && scratch && totals && mask_start && edge_start && counts, "null pointer");
    Lists L;
    lists_layout((void*)scratch, blocks, &L);
    lists_fill_kernel<<<(unsigned)blocks, DT, 0, (hipStream_t)stream>>>(F, bpf, N, mask, mask_i, mask_o, L.mstart, L.estart, totals, mask_start,
                                                                       edge_start, counts, mask_loc, edge_loc);
    return ia::check_launch("ia_flag_lists_fill");
}

IA_EXPORT int ia_sample_batch(int64_t n, int64_t num_mask, int64_t num_edge, int64_t frame, int64_t F, int H, int W, const int64_t* words,
                              const float* masks, const uint8_t* images, const int32_t* mask_start, const int32_t* edge_start,
                              const int32_t* mask_loc, const int32_t* edge_loc, const double* cam_host, const float* near_tab,
                              const float* far_tab, int64_t* indices, float* alpha, float* rgb, float* rays_o, float* rays_d, float* near,
                              float* far, int32_t* status, ia_stream_t stream)
{
    IA_REQUIRE(H > 0 && W > 0 && (int64_t)H * W <= INT32_MAX, "bad image size");
    IA_REQUIRE(frame >= 0 && frame < F, "frame index outside the set");
    IA_REQUIRE(num_mask >= 0 && num_edge >= 0 && num_mask + num_edge <= n, "bad split of the rows");
    IA_REQUIRE(words || (num_mask == 0 && num_edge == 0 && n <= (int64_t)H * W), "without words the rows are the frame's first n pixels");
    IA_REQUIRE(num_mask == 0 || (mask_start && mask_loc), "rows from the mask list need the list");
    IA_REQUIRE(num_edge == 0 || (edge_start && edge_loc), "rows from the edge list need the list");
    IA_REQUIRE(masks && images && cam_host && near_tab && far_tab && status, "null pointer");
    IA_REQUIRE(n == 0 || (indices && alpha && rgb && rays_o && rays_d && near && far), "null pointer");
    IA_REQUIRE((n + DT - 1) / DT <= INT32_MAX, "too many rows");
    const unsigned blocks = n > 0 ? (unsigned)((n + DT - 1) / DT) : 1u;       // n = 0 still reports the status
    sample_kernel<<<blocks, DT, 0, (hipStream_t)stream>>>(n, num_mask, num_edge, frame, (int64_t)H * W, W, words, masks, images, mask_start,
                                                         edge_start, mask_loc, edge_loc, load_cam(cam_host), near_tab, far_tab, indices, alpha,
                                                         rgb, rays_o, rays_d, near, far, status);
    return ia::check_launch("ia_sample_batch");
}

IA_EXPORT int ia_truth_valid_rect(int64_t F, int H, int W, const float* masks, int k, int32_t* rect, ia_stream_t stream)
{
    IA_REQUIRE(H > 0 && W > 0 && (int64_t)H * W <= INT32_MAX, "bad image size");
    IA_REQUIRE(k >= 1 && F >= 0 && F <= INT32_MAX, "need a window of at least one tap and a frame count below 2^31");
    if (F == 0) return IA_OK;
    IA_REQUIRE(masks && rect, "null pointer");
    valid_rect_kernel<<<(unsigned)F, DT, 0, (hipStream_t)stream>>>(H, W, k, masks, rect);
    return ia::check_launch("ia_truth_valid_rect");
}

IA_EXPORT int ia_sample_truth(int64_t n, int64_t frame, int64_t F, int H, int W, const int64_t* pixel_indices, const uint8_t* albedos,
                              const uint8_t* normals, const int32_t* rect, float* albedo, float* normal, uint8_t* valid, ia_stream_t stream)
{
    IA_REQUIRE(H > 0 && W > 0 && (int64_t)H * W <= INT32_MAX, "bad image size");
    IA_REQUIRE(frame >= 0 && frame < F, "frame index outside the set");
    IA_REQUIRE(n >= 0 && (pixel_indices || n <= (int64_t)H * W), "without pixel indices the rows are the frame's first n pixels");
    if (n == 0) return IA_OK;
    IA_REQUIRE(albedos && normals && rect && albedo && normal && valid, "null pointer");
    IA_REQUIRE((n + DT - 1) / DT <= INT32_MAX, "too many rows");
    sample_truth_kernel<<<(unsigned)((n + DT - 1) / DT), DT, 0, (hipStream_t)stream>>>(n, frame, (int64_t)H * W, W, pixel_indices, albedos, normals,
                                                                                       rect, albedo, normal, valid);
    return ia::check_launch("ia_sample_truth");
}

IA_EXPORT int ia_downscale_center_u8(int64_t F, int H, int W, int C, int s, const uint8_t* in, uint8_t* out, ia_stream_t stream)
{
    return downscale_center<uint8_t>("ia_downscale_center_u8", F, H, W, C, s, in, out, stream);
}

IA_EXPORT int ia_downscale_center_f32(int64_t F, int H, int W, int s, const float* in, float* out, ia_stream_t stream)
{
    return downscale_center<float>("ia_downscale_center_f32", F, H, W, 1, s, in, out, stream);
}
