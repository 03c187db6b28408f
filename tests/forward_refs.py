"""Plain torch references of the forward field kernels (csrc/mlp.hip, csrc/mlp_tile.h, ia_sh4_fwd, the level-major layouts of the
hash gather), their input generators, the size constants of tests/test_gpu_forward_kernels.py and the prefix form of the
comparison rule.

Nothing here touches the GPU or imports the library.  The convention is the one of tests/backward_refs.py: every reference is
ONE formula that runs in the dtype of its inputs -- fed the fp32 inputs cast up it is `ref64`, fed them as they are it is `twin32`
-- and the only tolerance is backward_refs.compare's  max|got - ref64| <= max(16 * e32, 32 ulp of max|ref64|).  The ReLU MLP
formula, its repaired generator, the segment spec and SH4 are backward_refs' own (mlp2_forward, make_mlp2_problem, MLP2_SPEC, sh4).

Prefix rule: a forward row depends on its own inputs only, so a case with n < PREFIX_ROWS is the first n rows of the
PREFIX_ROWS-row problem of the same seed; e32, the scale and the floor are taken over ALL rows of that problem (compare_rows), the
kernel runs on the contiguous prefix.  A one-row, one-column output does not get a bar set by one chance cancellation that way.
"""
import functools
import math

import torch
import torch.nn.functional as F

from tests import backward_refs as BR

F32, F64 = torch.float32, torch.float64

# ----------------------------------------------------------------------------------------------------------------------
# sizes.  Every forward MLP kernel works on 32-row tiles, one tile per wave and loop iteration.
#
# ia_mlp_fwd and ia_sdf_levels_fwd_grad (launch_fwd): at most 256 workgroups of 12 waves, so one round of the grid-stride loop is
# 256 * 12 * 32 = 98 304 rows (backward_refs.N_BIG = 65 637 stays inside it).  1 / 31 / 32 / 33 / 63 / 65: a ragged, a full and a
# just-started tile, one and two waves; 383 / 384 / 385: around one full workgroup (12 * 32 rows), 385 starts a second one with a
# one-row tile; 98 341 = 98 304 + 37: tiles 3072 and 3073 are the SECOND iteration of waves 0 and 1 of workgroup 0, the last a
# ragged 5-row tile, every other wave leaves the loop after one.
MLP_ROUND = 256 * 12 * 32
MLP_NS = (1, 31, 32, 33, 63, 65, 383, 384, 385, MLP_ROUND + 37)
MLP_WIDE_NS = (33, 385, MLP_ROUND + 37)          # the `wide` Softplus regime runs at these
MLP_LAYOUT_NS = (33, MLP_ROUND + 37)             # the three extra source layouts run at these
# ia_sdf_levels_fwd: the default kernel runs 256 workgroups of 16 waves, one round = 256 * 16 * 32 = 131 072 rows.  Its software
# pipeline keeps tile t, t + round and t + 2 rounds in flight; prologue, the two unrolled loop halves and the exit differ by how
# many tiles a wave owns.  n = k * 131 072 + 33 (k = 1 .. 4): 4096 k + 2 tiles, so waves 0 and 1 own k + 1 tiles (2 .. 5), every
# other wave owns k (1 .. 4), and the last tile holds ONE row.  The 12- and 8-wave variants (rounds of 98 304 and 65 536 rows) own
# up to 6 and 9 tiles per wave at the same sizes.  The small sizes are a single wave with one or two ragged / full tiles.
VALUE_ROUND = 256 * 16 * 32
VALUE_NS = (1, 31, 32, 33, 65) + tuple(k * VALUE_ROUND + 33 for k in (1, 2, 3, 4))
VALUE_WIDE_NS = (33, 2 * VALUE_ROUND + 33)
VALUE_KERNELS = (None, "pipe2w12", "pipe2w8", "pipe12", "pipe8", "tile")         # values of IA_SDF_HEAD (None: unset, the default)
# ia_sh4_fwd: one lane per row, 256-thread workgroups; N_BIG is more than one workgroup per CU
SH_NS = (1, 255, 256, 257, BR.N_BIG)

PREFIX_ROWS = 257


def problem_rows(n):
    """rows of the problem that case `n` is (a prefix of)."""
    return max(int(n), PREFIX_ROWS)


def compare_rows(what, got, ref64, twin32, factor=BR.FACTOR):
    """backward_refs.compare for a kernel run on the first got.shape[0] rows of a problem: e32, scale and floor over ALL rows of
    ref64 / twin32, the error over the rows the kernel computed; the same inequality, the same table row."""
    got, ref64, twin32 = BR._d(got), BR._d(ref64), BR._d(twin32)
    n = got.shape[0]
    assert ref64.shape == twin32.shape and n <= ref64.shape[0] and got.shape == ref64[:n].shape, (what, got.shape, ref64.shape, twin32.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite kernel result"
    scale = float(ref64.abs().max())
    err = float((got - ref64[:n]).abs().max())
    e32 = float((twin32 - ref64).abs().max())
    floor = BR.FLOOR_ULPS * 2.0 ** -23 * scale
    ratio = err / e32 if e32 > 0 else math.inf if err > 0 else 0.0
    BR.TABLE.append((what, err, e32, ratio))
    print(f"CMP {what:<44s} err {err:9.3e}  e32 {e32:9.3e}  err/e32 {ratio:8.2f}  max|ref| {scale:9.3e}")
    assert scale > 0.0, f"{what}: vacuous comparison (the reference is all zero)"
    assert err <= max(factor * e32, floor), (what, err, e32, ratio, floor)


# ----------------------------------------------------------------------------------------------------------------------
# SDF head 35 -> 64 (Softplus beta = 100) -> 13 with the analytic gradient, forward
SDF_CENTER = (0.1, -0.2, 0.05)
SDF_EXTENT = (2.1, 2.6, 1.9)           # non-uniform: a swapped axis of 1 / extent shows in the gradient
SDF_FWD_SEED = 1
# scale of W1 / b1.  narrow: z = h W1^T + b1 mostly inside the Softplus knee (|100 z| < 9.2: log1p taken from the logarithm); wide:
# a fifth of the units on each saturated side (100 z > 20: the pass-through; 100 z < -20: exp(-|100 z|) < 2e-9) and a tenth in
# 9.2 < |100 z| <= 20, where softplus100's e < 1e-4 branch switches
SDF_W1_SCALES = {"narrow": BR.SDF_W1_SCALE, "wide": 0.15}


def inv_scale():
    """the kernels' `inv_scale` argument: 1 / extent, per axis."""
    return tuple(1.0 / s for s in SDF_EXTENT)


def make_sdf_fwd_problem(rows, regime, seed=SDF_FWD_SEED, with_jac=True):
    """fp32 inputs of the SDF head: weights first (the same for every `rows`), then enc [rows,32] and x [rows,3] uniform in [0,1],
    the Jacobian [rows,32,3] last (with_jac = False draws the same everything else)."""
    g = BR.seeded(seed)
    sc = SDF_W1_SCALES[regime]
    p = dict(n=rows, regime=regime, W1=BR.randn(g, 64, 35, scale=sc), b1=BR.randn(g, 64, scale=sc), W2=BR.randn(g, 13, 64),
             b2=BR.randn(g, 13), enc=BR.randn(g, rows, 32), x=torch.rand(rows, 3, generator=g))
    p["jac"] = BR.randn(g, rows, 32, 3) if with_jac else None
    return p


def sdf_preactivation(p, dtype=F64):
    h = torch.cat([p["enc"].to(dtype), 2.0 * p["x"].to(dtype) - 1.0], -1)
    return h @ p["W1"].to(dtype).T + p["b1"].to(dtype)


def sdf_fwd_regime_shares(p):
    """shares of the (row, unit) pairs, in fp64: (|100 z| < 9.2, 100 z > 20, 100 z < -20, 9.2 < |100 z| <= 20)."""
    bz = 100.0 * sdf_preactivation(p)
    m = lambda c: float(c.double().mean())      # noqa: E731
    return m(bz.abs() < 9.2), m(bz > 20), m(bz < -20), m((bz.abs() > 9.2) & (bz.abs() <= 20))


def sdf_fwd_ref(p, dtype):
    """VolumeSDF.forward on world points pts, centre c, extent s:  x = (pts - c) / s + 0.5,  h = [enc + J (x - x.detach()), 2 x - 1],
    out = softplus(h W1^T + b1, beta = 100) W2^T + b2,  grad = d out[:,0].sum() / d pts by autograd (None without a Jacobian).
    The kernels are handed x, not pts: pts is formed from the shared fp32 x and the VALUE of x in h is that input itself (the
    normalisation adds x_of_pts - x_of_pts.detach(), an exact zero that carries d x / d pts = 1 / s)."""
    t = lambda k: p[k].to(dtype)      # noqa: E731
    c, s = torch.tensor(SDF_CENTER, dtype=dtype), torch.tensor(SDF_EXTENT, dtype=dtype)
    want_grad = p["jac"] is not None
    pts = ((t("x") - 0.5) * s + c).requires_grad_(want_grad)
    xn = (pts - c) / s + 0.5
    x = t("x") + (xn - xn.detach())
    enc = t("enc") + torch.einsum("nkc,nc->nk", t("jac"), x - x.detach()) if want_grad else t("enc")
    h = torch.cat([enc, 2.0 * x - 1.0], -1)
    out = F.softplus(h @ t("W1").T + t("b1"), beta=100) @ t("W2").T + t("b2")
    grad = torch.autograd.grad(out[:, 0].sum(), pts)[0] if want_grad else None
    return dict(out=out.detach(), grad=grad)


def sdf_fwd_closed_form(p, dtype=F64):
    """second opinion only (what the kernel's epilogue implements): grad = (J^T g_h[:32] + 2 g_h[32:35]) / s with
    g_h = (softplus'(z) W2[0]) W1; softplus' of Softplus(beta = 100, threshold = 20) is sigmoid(100 z) up to the threshold and 1
    above it (where 1 - sigmoid < 2.1e-9)."""
    z = sdf_preactivation(p, dtype)
    sg = torch.where(100.0 * z > 20.0, torch.ones_like(z), torch.sigmoid(100.0 * z))
    gh = (sg * p["W2"].to(dtype)[0]) @ p["W1"].to(dtype)
    return (torch.einsum("nkc,nk->nc", p["jac"].to(dtype), gh[:, :32]) + 2.0 * gh[:, 32:35]) / torch.tensor(SDF_EXTENT, dtype=dtype)


@functools.lru_cache(maxsize=None)
def sdf_head_case(rows, regime):
    """(problem, ref64, twin32) of the full head with gradient (sections B and C of the GPU file)."""
    p = make_sdf_fwd_problem(rows, regime)
    return p, sdf_fwd_ref(p, F64), sdf_fwd_ref(p, F32)


@functools.lru_cache(maxsize=None)
def sdf_value_case(rows, regime):
    """(problem, ref64 out[:,0], twin32 out[:,0]) without a Jacobian (section D): the same weights, enc and x as sdf_head_case."""
    p = make_sdf_fwd_problem(rows, regime, with_jac=False)
    return p, sdf_fwd_ref(p, F64)["out"][:, 0].clone(), sdf_fwd_ref(p, F32)["out"][:, 0].clone()


def sdf_head_cases():
    """(n, regime) of sections B and C."""
    return [(n, "narrow") for n in MLP_NS] + [(n, "wide") for n in MLP_WIDE_NS]


def sdf_value_cases():
    """(n, regime) of section D."""
    return [(n, "narrow") for n in VALUE_NS] + [(n, "wide") for n in VALUE_WIDE_NS]


# ----------------------------------------------------------------------------------------------------------------------
# the level-major layouts of the hash gather: features float2 [16][n], Jacobian float [16][n][6]
def to_levels(enc):
    """[n,32] -> [16,n,2]: element [l][p][f] is feature 2 l + f of point p."""
    n = enc.shape[0]
    return enc.reshape(n, 16, 2).permute(1, 0, 2).contiguous()


def from_levels(lv):
    n = lv.shape[1]
    return lv.permute(1, 0, 2).reshape(n, 32).contiguous()


def to_levels_jac(jac):
    """[n,32,3] -> [16,n,6]: element [l][p][f * 3 + axis] is d feature (2 l + f) / d x_axis of point p."""
    n = jac.shape[0]
    return jac.reshape(n, 16, 6).permute(1, 0, 2).contiguous()


def from_levels_jac(lj):
    n = lj.shape[1]
    return lj.permute(1, 0, 2).reshape(n, 32, 3).contiguous()


# ----------------------------------------------------------------------------------------------------------------------
# ReLU MLPs with a sigmoid output (kinds 1 and 2), forward
MLP2_FWD_SEED = 1
SATURATION_GAIN = 40.0               # Wo and bo times this: z3 far out on both sides of the sigmoid
SATURATED_CASE = (257, 1)            # (n, seed)


@functools.lru_cache(maxsize=None)
def mlp2_problem(kind, rows, seed=MLP2_FWD_SEED, zero_units=False, saturated=False):
    p = BR.make_mlp2_problem(kind, rows, seed, zero_units=zero_units)
    if saturated:
        p["weights"] = p["weights"][:4] + [p["weights"][4] * SATURATION_GAIN, p["weights"][5] * SATURATION_GAIN]
    return p


def mlp2_fwd_ref(kind, p, dtype):
    f = BR.mlp2_forward(kind, [s.to(dtype) for s in p["segs"]], *[w.to(dtype) for w in p["weights"]])
    return dict(y=f["y"], z3=f["z3"])


@functools.lru_cache(maxsize=None)
def mlp2_case(kind, rows, seed=MLP2_FWD_SEED, zero_units=False, saturated=False):
    p = mlp2_problem(kind, rows, seed, zero_units, saturated)
    return p, mlp2_fwd_ref(kind, p, F64), mlp2_fwd_ref(kind, p, F32)


# ----------------------------------------------------------------------------------------------------------------------
# SH4
SH_SEED = 3
SH_SPECIAL = ((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0),
              (3.0 ** -0.5, 3.0 ** -0.5, 3.0 ** -0.5))


def make_sh_fwd_problem(rows, seed=SH_SEED):
    """d01 = (d + 1) / 2 of unit directions d: normalised randn, the first rows the six axis directions and (1,1,1) / sqrt 3."""
    g = BR.seeded(seed)
    d = F.normalize(BR.randn(g, rows, 3, scale=1.0), dim=-1)
    k = min(rows, len(SH_SPECIAL))
    d[:k] = torch.tensor(SH_SPECIAL)[:k]
    return dict(n=rows, d01=(d + 1.0) / 2.0)


@functools.lru_cache(maxsize=None)
def sh_case(rows):
    p = make_sh_fwd_problem(rows)
    return p, BR.sh4(p["d01"].double()), BR.sh4(p["d01"])


# ----------------------------------------------------------------------------------------------------------------------
# points of the gather's layout test
HASH_SPECIAL = ((0, 0, 0), (1, 1, 1), (0.5, 0.5, 0.5), (0, 1, 0), (1, 0, 0), (0.999999, 0.5, 0.25), (1e-7, 0.3, 0.9), (0.25, 0.25, 0.25))


def make_hash_points(n, seed=7):
    """uniform in [0,1] with the eight special points of the bit-for-bit gather test (corners, centre, faces, next to a face) first."""
    x = torch.rand(n, 3, generator=BR.seeded(seed))
    x[:len(HASH_SPECIAL)] = torch.tensor(HASH_SPECIAL, dtype=F32)
    return x
