// occgrid.hip -- per-frame occupancy-grid maintenance for gfx950.
// Replaces the torch op chains of
//   TemporalOccGridEstimator._update          models/occ_grid/temporal_occ_grid.py:369-411
//   IntrinsicAvatarModel._compute_occupancy_grid  models/intrinsic_avatar.py:307-358
//   max_connected_component                   models/utils.py:152-163   (192 x F.max_pool3d on a 64^3 float grid)
// Stages: EMA (max(decayed, new)) -> 3^3 max-pool dilation -> mean-clamped threshold -> binary grid ->
// connected components by label propagation (26-connectivity, exactly res*3 synchronous sweeps like the
// reference, so partially converged labels match too) -> keep the most frequent label.
// Grids are tiny (64^3 = 1 MB of labels): every kernel is one lane per cell; the whole rebuild is ~200 short
// launches (~1 ms) instead of ~200 library pooling calls.
#include "ia_common.h"

namespace {

constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void ema_kernel(int64_t n, float* __restrict__ occs, const float* __restrict__ occ_new,
                                                       float decay)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i < n) occs[i] = fmaxf(occs[i] * decay, occ_new[i]);
}

// 3x3x3 max-pool (stride 1, -inf padding) + deterministic partial sums of the pooled values >= 0
__global__ __launch_bounds__(THREADS) void dilate_kernel(int rx, int ry, int rz, const float* __restrict__ occs,
                                                          float* __restrict__ pooled, double* __restrict__ part_sum,
                                                          int64_t* __restrict__ part_cnt)
{
    __shared__ double s_sum[THREADS];
    __shared__ int s_cnt[THREADS];
    const int64_t n = (int64_t)rx * ry * rz;
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    double v_sum = 0.0;
    int v_cnt = 0;
    if (c < n) {
        const int z = (int)(c % rz), y = (int)((c / rz) % ry), x = (int)(c / ((int64_t)ry * rz));
        float m = -INFINITY;
        for (int dx = -1; dx <= 1; dx++)
            for (int dy = -1; dy <= 1; dy++)
                for (int dz = -1; dz <= 1; dz++) {
                    const int xx = x + dx, yy = y + dy, zz = z + dz;
                    if (xx < 0 || xx >= rx || yy < 0 || yy >= ry || zz < 0 || zz >= rz) continue;
                    m = fmaxf(m, occs[((int64_t)xx * ry + yy) * rz + zz]);
                }
        pooled[c] = m;
        if (m >= 0.0f) { v_sum = (double)m; v_cnt = 1; }
    }
    s_sum[threadIdx.x] = v_sum;
    s_cnt[threadIdx.x] = v_cnt;
    __syncthreads();
    for (int off = THREADS / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) { s_sum[threadIdx.x] += s_sum[threadIdx.x + off]; s_cnt[threadIdx.x] += s_cnt[threadIdx.x + off]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part_sum[blockIdx.x] = s_sum[0]; part_cnt[blockIdx.x] = s_cnt[0]; }
}

// thre = min(mean, thre_max); binaries = pooled > thre   (one block finishes the reduction in a fixed order)
__global__ __launch_bounds__(THREADS) void threshold_kernel(int64_t n, int n_parts, const float* __restrict__ pooled,
                                                             const double* __restrict__ part_sum,
                                                             const int64_t* __restrict__ part_cnt, float thre_max,
                                                             uint8_t* __restrict__ binaries, float* __restrict__ thre_out)
{
    __shared__ float s_thre;
    if (threadIdx.x == 0) {
        double s = 0.0;
        int64_t k = 0;
        for (int i = 0; i < n_parts; i++) { s += part_sum[i]; k += part_cnt[i]; }
        const float mean = k > 0 ? (float)(s / (double)k) : NAN;
        s_thre = mean < thre_max ? mean : thre_max;            // torch.clamp(mean, max=thre_max); NaN stays NaN
        if (blockIdx.x == 0 && thre_out) *thre_out = s_thre;
    }
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (c < n) binaries[c] = pooled[c] > s_thre ? 1 : 0;
}

__global__ __launch_bounds__(THREADS) void cc_init_kernel(int64_t n, const uint8_t* __restrict__ binaries,
                                                           int32_t* __restrict__ labels)
{
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (c < n) labels[c] = binaries[c] ? (int32_t)(c + 1) : 0;
}

// one synchronous sweep: label <- max over the 3^3 neighbourhood (zero padding), masked by the grid
__global__ __launch_bounds__(THREADS) void cc_step_kernel(int rx, int ry, int rz, const uint8_t* __restrict__ binaries,
                                                           const int32_t* __restrict__ in, int32_t* __restrict__ out)
{
    const int64_t n = (int64_t)rx * ry * rz;
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (c >= n) return;
    if (!binaries[c]) { out[c] = 0; return; }
    const int z = (int)(c % rz), y = (int)((c / rz) % ry), x = (int)(c / ((int64_t)ry * rz));
    int32_t m = 0;
    for (int dx = -1; dx <= 1; dx++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dz = -1; dz <= 1; dz++) {
                const int xx = x + dx, yy = y + dy, zz = z + dz;
                if (xx < 0 || xx >= rx || yy < 0 || yy >= ry || zz < 0 || zz >= rz) continue;
                m = max(m, in[((int64_t)xx * ry + yy) * rz + zz]);
            }
    out[c] = m;
}

__global__ __launch_bounds__(THREADS) void cc_hist_kernel(int64_t n, const int32_t* __restrict__ labels,
                                                           int32_t* __restrict__ hist)
{
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (c < n && labels[c] > 0) atomicAdd(&hist[labels[c]], 1);
}

// most frequent label (ties -> smallest label, like torch.mode); single block, fixed order
__global__ __launch_bounds__(1024) void cc_argmax_kernel(int64_t n, const int32_t* __restrict__ hist, int32_t* __restrict__ best)
{
    __shared__ int s_cnt[1024];
    __shared__ int s_lab[1024];
    int bc = 0, bl = 0;
    for (int64_t l = 1 + threadIdx.x; l <= n; l += 1024) {
        const int h = hist[l];
        if (h > bc) { bc = h; bl = (int)l; }          // ascending scan: first (smallest) label wins ties
    }
    s_cnt[threadIdx.x] = bc;
    s_lab[threadIdx.x] = bl;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if (threadIdx.x < off) {
            const int oc = s_cnt[threadIdx.x + off], ol = s_lab[threadIdx.x + off];
            if (oc > s_cnt[threadIdx.x] || (oc == s_cnt[threadIdx.x] && oc > 0 && ol < s_lab[threadIdx.x])) {
                s_cnt[threadIdx.x] = oc;
                s_lab[threadIdx.x] = ol;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *best = s_lab[0];
}

__global__ __launch_bounds__(THREADS) void cc_select_kernel(int64_t n, const int32_t* __restrict__ labels,
                                                             const int32_t* __restrict__ best, uint8_t* __restrict__ binaries)
{
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (c < n) binaries[c] = (labels[c] == *best) ? 1 : 0;        // (mcc == label), incl. 0 == 0 when the grid is empty
}

}  // namespace

IA_EXPORT int ia_occgrid_ema(int64_t n_cells, float* occs, const float* occ_new, float ema_decay, ia_stream_t stream)
{
    if (n_cells == 0) return IA_OK;
    ema_kernel<<<ia::cdiv(n_cells, THREADS), THREADS, 0, (hipStream_t)stream>>>(n_cells, occs, occ_new, ema_decay);
    return ia::check_launch("ia_occgrid_ema");
}

// pooled f32[n] | labels A i32[n] | labels B i32[n] | hist i32[n+2] | part_sum f64[parts] | part_cnt i64[parts] | best; tmp 4-byte aligned
struct BinarizeTmp {
    float* pooled;
    int32_t *labA, *labB, *hist;
    double* part_sum;
    int64_t* part_cnt;
    int32_t* best;
};

static size_t binarize_layout(void* tmp, int64_t n, BinarizeTmp* t)
{
    const size_t cells = (size_t)(n > 0 ? n : 0), parts = (cells + THREADS - 1) / THREADS;
    ia::Carver c(tmp);
    t->pooled = c.take<float>(cells, 4);
    t->labA = c.take<int32_t>(cells, 4);
    t->labB = c.take<int32_t>(cells, 4);
    t->hist = c.take<int32_t>(cells + 2, 4);
    t->part_sum = c.take<double>(parts, 16);
    t->part_cnt = c.take<int64_t>(parts, 8);
    t->best = c.take<int32_t>(1, 4);
    c.skip(64);                                          // tail slack, as the callers have always allocated
    return c.need(4);
}

IA_EXPORT int64_t ia_occgrid_tmp_bytes(int rx, int ry, int rz)
{
    BinarizeTmp t;
    return (int64_t)binarize_layout(nullptr, (int64_t)rx * ry * rz, &t);
}

IA_EXPORT int ia_occgrid_binarize(int rx, int ry, int rz, const float* occs, float thre_max, int keep_largest_component,
                                  uint8_t* binaries, float* thre_out, void* tmp, ia_stream_t stream)
{
    IA_REQUIRE(rx > 0 && ry > 0 && rz > 0, "grid resolution must be positive");
    const int64_t n = (int64_t)rx * ry * rz;
    const int grid = ia::cdiv(n, THREADS);
    hipStream_t s = (hipStream_t)stream;
    BinarizeTmp t;
    binarize_layout(tmp, n, &t);
    float* pooled = t.pooled;
    int32_t *labA = t.labA, *labB = t.labB, *hist = t.hist, *best = t.best;
    double* part_sum = t.part_sum;
    int64_t* part_cnt = t.part_cnt;
    dilate_kernel<<<grid, THREADS, 0, s>>>(rx, ry, rz, occs, pooled, part_sum, part_cnt);
    threshold_kernel<<<grid, THREADS, 0, s>>>(n, grid, pooled, part_sum, part_cnt, thre_max, binaries, thre_out);
    if (keep_largest_component) {
        cc_init_kernel<<<grid, THREADS, 0, s>>>(n, binaries, labA);
        const int sweeps = rz * 3;                                   // models/utils.py:160
        for (int it = 0; it < sweeps; it++) {
            cc_step_kernel<<<grid, THREADS, 0, s>>>(rx, ry, rz, binaries, labA, labB);
            int32_t* t = labA; labA = labB; labB = t;
        }
        if (hipMemsetAsync(hist, 0, sizeof(int32_t) * (n + 2), s) != hipSuccess) { ia::set_error("memset failed"); return IA_ERR_LAUNCH; }
        cc_hist_kernel<<<grid, THREADS, 0, s>>>(n, labA, hist);
        cc_argmax_kernel<<<1, 1024, 0, s>>>(n, hist, best);
        cc_select_kernel<<<grid, THREADS, 0, s>>>(n, labA, best, binaries);
    }
    return ia::check_launch("ia_occgrid_binarize");
}
