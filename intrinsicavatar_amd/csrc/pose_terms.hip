// pose_terms.hip -- backward of the two places the bone transforms enter the training graph (SNARFDeformer.implicit_pose_terms,
// deformer.py; ForwardDeformer.forward version 1, deformer_torch.py:57-76, and SNARFDeformer.deform_, snarf_deformer.py:176-184):
//
//     w_p      = the 24 trilinear weights of ia_forward_skinning at xc_p            (ia_lbs_weights of lbs_math.h: the same bits)
//     gx_p     = -valid_p * J_inv_p^T g_pts_p
//     G_p[3,4] = [ valid_p * g_c2w_p + gx_p xc_p^T | gx_p ]
//     g_tfs[j][:3,:4] = sum_p w_p[j] * G_p ,   g_tfs[j][3,:] = 0
//
// a [24 x P] . [P x 12] product whose left operand is looked up and whose right operand is formed on the way: neither is written to
// memory.  Built with -ffp-contract=off (the weights must be ia_forward_skinning's).
//
// pose_terms_partial_kernel: one point per lane, 256 per tile, a block walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ...  Per tile
// every lane leaves its 24 weights (fp32, row stride 25 words) and its 12 entries of G (fp64, formed in fp64 from the fp32 inputs, row
// stride 13) in LDS; then lane t owns output t = 12 j + e (lanes 0 .. 31 also output 256 + t) and walks the tile's points in ascending
// order: acc += (double)w[q][j] * G[q][e].  Inside a wave the reads of a point touch 6 weights and 12 entries of G: broadcasts, no bank
// conflict.  An invalid point (and a lane past P) loads no grid corner and stores zeros.  The block's 288 fp64 sums go to
// partials[288][n_blocks] (output-major: the second pass reads rows); pose_terms_finish_kernel, one wave per output, has lane l add the
// blocks l, l + 64, ... in ascending order, lane 0 add the 64 lane sums in ascending order, and rounds once to fp32.  No atomics: the
// number of blocks is a function of P alone (one tile per block up to 2048 tiles = 524 288 points, a strided walk beyond), every sum
// has one fixed order, two calls give the same bits.  The product of two fp32 numbers is exact in fp64, so the only rounding beyond the
// inputs' is the fp64 summation (2^-53 per step) and the final cast.
// What bounds it: the gather -- 192 words per valid point from the L2 / Infinity-Cache resident grid, as in lbs_fwd.hip; the
// reduction adds 288 fp64 multiply-adds and about 2.3 LDS words per point and output lane.
#include "ia_common.h"
#include "lbs_math.h"

namespace {

constexpr int PT_WG = 256;
constexpr int PT_WROW = IA_LBS_BONES + 1;       // fp32 words per point in LDS
constexpr int PT_GROW = 13;                     // fp64 words per point in LDS
constexpr int PT_OUT = IA_LBS_BONES * 12;       // 288 sums
constexpr int PT_MAX_BLOCKS = 2048;

struct PoseTermsTmp {
    double* partials;                           // [288, n_blocks]
};

int pose_terms_blocks(int64_t P)
{
    const int64_t tiles = (P + PT_WG - 1) / PT_WG;
    return (int)(tiles < PT_MAX_BLOCKS ? tiles : PT_MAX_BLOCKS);
}

size_t pose_terms_layout(void* tmp, int64_t P, PoseTermsTmp* t)
{
    ia::Carver c(tmp);
    t->partials = c.take<double>((size_t)pose_terms_blocks(P) * PT_OUT, 8);
    return c.need(8);
}

__global__ __launch_bounds__(PT_WG) void pose_terms_partial_kernel(int64_t P, const float* __restrict__ xc, const float* __restrict__ J_inv,
                                                                    const int64_t* __restrict__ win, int64_t n_jinv,
                                                                    const uint8_t* __restrict__ valid, const float* __restrict__ g_pts,
                                                                    const float* __restrict__ g_c2w, const float* __restrict__ grid, int D, int H,
                                                                    int W, const float* __restrict__ offset, const float* __restrict__ scale,
                                                                    double* __restrict__ partials)
{
    __shared__ float sw[PT_WG * PT_WROW];
    __shared__ double sg[PT_WG * PT_GROW];
    const int lane = threadIdx.x;
    const int j0 = lane / 12, e0 = lane - 12 * j0;                  // output lane
    const int o1 = PT_WG + lane;                                    // second output of lanes 0 .. 31
    const bool two = o1 < PT_OUT;
    const int j1 = two ? o1 / 12 : 0, e1 = two ? o1 - 12 * j1 : 0;
    double acc0 = 0.0, acc1 = 0.0;
    const int64_t tiles = (P + PT_WG - 1) / PT_WG;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t base = tile * PT_WG;
        const int64_t p = base + lane;
        float w[IA_LBS_BONES];
        double G[12];
        bool on = p < P && valid[p] != 0;
        int64_t q = 0;
        if (on) {
            q = win ? win[p] : p;
            on = q >= 0 && q < n_jinv;                              // an index outside the J_inv list contributes nothing
        }
        if (on) {
            const float x[3] = {xc[3 * p], xc[3 * p + 1], xc[3 * p + 2]};
            ia_lbs_weights(x, grid, D, H, W, offset, scale, w);
            const float* Ji = J_inv + 9 * q;
            const double gp[3] = {g_pts[3 * p], g_pts[3 * p + 1], g_pts[3 * p + 2]};
#pragma unroll
            for (int r = 0; r < 3; r++) {
                // gx_r = -(J_inv^T g_pts)_r
                const double gx = -((double)Ji[r] * gp[0] + (double)Ji[3 + r] * gp[1] + (double)Ji[6 + r] * gp[2]);
#pragma unroll
                for (int c = 0; c < 3; c++) G[4 * r + c] = (double)g_c2w[9 * p + 3 * r + c] + gx * (double)x[c];
                G[4 * r + 3] = gx;
            }
        } else {
#pragma unroll
            for (int j = 0; j < IA_LBS_BONES; j++) w[j] = 0.0f;
#pragma unroll
            for (int e = 0; e < 12; e++) G[e] = 0.0;
        }
#pragma unroll
        for (int j = 0; j < IA_LBS_BONES; j++) sw[lane * PT_WROW + j] = w[j];
#pragma unroll
        for (int e = 0; e < 12; e++) sg[lane * PT_GROW + e] = G[e];
        __syncthreads();
        const int64_t left = P - base;
        const int count = (int)(left < PT_WG ? left : PT_WG);
        for (int k = 0; k < count; k++) {
            acc0 += (double)sw[k * PT_WROW + j0] * sg[k * PT_GROW + e0];
            if (two) acc1 += (double)sw[k * PT_WROW + j1] * sg[k * PT_GROW + e1];
        }
        __syncthreads();
    }
    partials[(int64_t)lane * gridDim.x + blockIdx.x] = acc0;
    if (two) partials[(int64_t)o1 * gridDim.x + blockIdx.x] = acc1;
}

// g_tfs [24,4,4], one wave per entry: rows 0 .. 2 = the sum of the blocks' partials (lane l the blocks l, l + 64, ... in ascending
// order, then lane 0 the 64 lane sums in ascending order), row 3 = 0
__global__ __launch_bounds__(ia::WAVE) void pose_terms_finish_kernel(int n_blocks, const double* __restrict__ partials, float* __restrict__ g_tfs)
{
    __shared__ double lane_sum[ia::WAVE];
    const int t = blockIdx.x;                       // < 24 * 16
    const int lane = threadIdx.x;
    const int j = t / 16, e = t - 16 * j;
    if (e >= 12) {
        if (lane == 0) g_tfs[t] = 0.0f;
        return;
    }
    const double* row = partials + (int64_t)(12 * j + e) * n_blocks;
    double s = 0.0;
    for (int b = lane; b < n_blocks; b += ia::WAVE) s += row[b];
    lane_sum[lane] = s;
    __syncthreads();
    if (lane == 0) {
        double tot = 0.0;
        for (int l = 0; l < ia::WAVE; l++) tot += lane_sum[l];
        g_tfs[t] = (float)tot;
    }
}

}  // namespace

IA_EXPORT int64_t ia_pose_terms_bwd_tmp_size(int64_t P)
{
    PoseTermsTmp t;
    return P > 0 ? (int64_t)pose_terms_layout(nullptr, P, &t) : 0;
}

IA_EXPORT int ia_pose_terms_bwd(int64_t P, const float* xc, const float* J_inv, const int64_t* win, int64_t n_jinv, const uint8_t* valid,
                                const float* g_pts, const float* g_c2w, const float* grid, int D, int H, int W, const float* offset,
                                const float* scale, float* g_tfs, void* tmp, ia_stream_t stream)
{
    IA_REQUIRE(P >= 0 && n_jinv >= 0, "negative count");
    IA_REQUIRE(g_tfs != nullptr, "g_tfs [24,4,4] is required");
    IA_REQUIRE(D >= 1 && H >= 1 && W >= 1 && (int64_t)D * H * W * IA_LBS_BONES <= INT32_MAX,
               "grid sides must be >= 1 and 24 * D * H * W must fit 31 bits");
    hipStream_t s = (hipStream_t)stream;
    int n_blocks = 0;
    PoseTermsTmp t{nullptr};
    if (P > 0) {
        IA_REQUIRE(xc && J_inv && valid && g_pts && g_c2w && grid && offset && scale, "null pointer");
        IA_REQUIRE(win != nullptr || n_jinv >= P, "without win, J_inv holds one matrix per point");
        IA_REQUIRE(tmp != nullptr && (reinterpret_cast<uintptr_t>(tmp) & 7) == 0, "tmp (ia_pose_terms_bwd_tmp_size, 8-byte aligned) is required");
        pose_terms_layout(tmp, P, &t);
        n_blocks = pose_terms_blocks(P);
        pose_terms_partial_kernel<<<n_blocks, PT_WG, 0, s>>>(P, xc, J_inv, win, n_jinv, valid, g_pts, g_c2w, grid, D, H, W, offset, scale,
                                                             t.partials);
    }
    pose_terms_finish_kernel<<<IA_LBS_BONES * 16, ia::WAVE, 0, s>>>(n_blocks, t.partials, g_tfs);
    return ia::check_launch("ia_pose_terms_bwd");
}
