// lbs_fwd.hip -- forward skinning of canonical points (ForwardDeformer.forward_skinning, deformer_torch.py:127-137): trilinear,
// border-clamped lookup of the 24-channel skinning-weight grid, blend of the 24 bone transforms, the skinned point and the blended
// rotation block.  The arithmetic lives in lbs_math.h (replayed on the host by tests/lbs_harness.c).  Built with -ffp-contract=off.
//
// lbs_forward_kernel: one point per lane, 256 per workgroup; a lane walks the 24 channels and loads its 8 corners of each (the x0 / x1
// corners of a pair are neighbouring words).  The grid is channel-major, so at one channel the 64 lanes of a wave read the cells of 64
// points: vertices of a marching-cubes mesh come out in grid order, neighbours in the array share or adjoin cells, and a wave's 8 loads
// of a channel land on a few cache lines of that channel's 2 MB plane (resolution 128) instead of 64 x 8.  The bone transforms are read
// through wave-uniform addresses.  The [256,24] block of weights goes through LDS (row stride 25 words: conflict-free) so that
// consecutive lanes store consecutive words; xd and R are 12 / 36 contiguous bytes per lane.  What bounds it: 192 gathered words per
// point against 12 B read and up to 144 B written -- the gather's cache-line traffic (L2 / Infinity Cache resident grid), not HBM
// and not arithmetic.  A point's result does not depend on P or on its place in the launch.
#include "ia_common.h"
#include "lbs_math.h"

namespace {

constexpr int LBS_WG = 256;
constexpr int LBS_ROW = IA_LBS_BONES + 1;

__global__ __launch_bounds__(LBS_WG) void lbs_forward_kernel(int64_t P, const float* __restrict__ xc, const float* __restrict__ grid, int D,
                                                              int H, int W, const float* __restrict__ offset, const float* __restrict__ scale,
                                                              const float* __restrict__ tfs, float* __restrict__ w_out,
                                                              float* __restrict__ xd_out, float* __restrict__ R_out)
{
    __shared__ float stage[LBS_WG * LBS_ROW];
    const int lane = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * LBS_WG;
    const bool live = base + lane < P;
    const int64_t p = live ? base + lane : P - 1;       // lanes past the end repeat the last point and write nothing
    const float x[3] = {xc[3 * p], xc[3 * p + 1], xc[3 * p + 2]};
    float w[IA_LBS_BONES];
    ia_lbs_weights(x, grid, D, H, W, offset, scale, w);
    if (xd_out || R_out) {                              // (uniform over the launch)
        float T[12];
        ia_lbs_blend(w, tfs, T);
        if (live && xd_out) {
#pragma unroll
            for (int r = 0; r < 3; r++) xd_out[3 * p + r] = ia_lbs_apply(T, x, r);
        }
        if (live && R_out) {
#pragma unroll
            for (int e = 0; e < 9; e++) R_out[9 * p + e] = T[4 * (e / 3) + e % 3];
        }
    }
    if (w_out) {                                        // (uniform over the launch)
#pragma unroll
        for (int j = 0; j < IA_LBS_BONES; j++) stage[lane * LBS_ROW + j] = w[j];
        __syncthreads();
        const int64_t left = P - base;
        const int total = (int)(left < LBS_WG ? left : LBS_WG) * IA_LBS_BONES;
        for (int f = lane; f < total; f += LBS_WG) {
            const int q = f / IA_LBS_BONES, j = f - q * IA_LBS_BONES;
            w_out[base * IA_LBS_BONES + f] = stage[q * LBS_ROW + j];
        }
    }
}

}  // namespace

IA_EXPORT int ia_forward_skinning(int64_t P, const float* xc, const float* grid, int D, int H, int W, const float* offset,
                                  const float* scale, const float* tfs, float* w, float* xd, float* R, ia_stream_t stream)
{
    IA_REQUIRE(P >= 0, "negative point count");
    IA_REQUIRE(D >= 1 && H >= 1 && W >= 1 && (int64_t)D * H * W * IA_LBS_BONES <= INT32_MAX,
               "grid sides must be >= 1 and 24 * D * H * W must fit 31 bits");
    if (P == 0 || (!w && !xd && !R)) return IA_OK;
    IA_REQUIRE(xc && grid && offset && scale, "null pointer");
    IA_REQUIRE(tfs || (!xd && !R), "xd and R need the bone transforms");
    IA_REQUIRE((P + LBS_WG - 1) / LBS_WG <= INT32_MAX, "too many points for one launch");
    lbs_forward_kernel<<<ia::cdiv(P, LBS_WG), LBS_WG, 0, (hipStream_t)stream>>>(P, xc, grid, D, H, W, offset, scale, tfs, w, xd, R);
    return ia::check_launch("ia_forward_skinning");
}
