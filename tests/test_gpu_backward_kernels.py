"""GPU: every training-backward kernel ALONE, with inputs of its own, against fp64 torch autograd of the same operation.

The whole-step gradient tests compare aggregated parameter gradients at 5e-3 of the largest entry; a wrong second-order term,
a ragged-tile mistake in the last rows, a mis-strided view or a dropped NULL-gradient branch stays far below that.  Here each
kernel is called through the route the training step uses (the torch.autograd.Function or the C ABI) and compared with
tests/backward_refs.py by the rule stated there:  max|got - ref64| <= max(16 * e32, 32 ulp of max|ref64|),  e32 = the error of
the same formula in fp32 on the CPU.  Pure copies / masks / gathers are compared with torch.equal.

The hash-grid TABLE backward (ia_hashgrid_bwd, ia_hashgrid_bwd_binned) is not here: its home is tests/test_gpu_hash_bwd_kernels.py
(same rule, applied per level; reference in tests/hash_bwd_refs.py).  This file stops at ia_hashgrid_jac_contract.

Measured on the MI355X (err = max|got - ref64|, e32 = max|twin32 - ref64|; the largest err/e32 per kernel and quantity over all
cases of this file, as backward_refs.format_table() prints it when the module's fixture is torn down):

    quantity                                           err       e32  err/e32   worst case
    mlp1 fused y                                  1.83e-07  5.56e-08     3.29   n=1
    mlp1 fused g_seg0                             8.68e-08  2.06e-08     4.21   n=1
    mlp1 fused g_seg1                             1.06e-07  3.79e-08     2.79   n=1
    mlp1 fused g_seg2                             7.25e-08  1.69e-08     4.28   n=1
    mlp1 fused g_seg3                             4.18e-08  1.96e-08     2.13   n=1
    mlp1 fused g_seg4                             5.29e-08  1.25e-08     4.24   n=1
    mlp1 fused dW1                                7.81e-08  2.63e-08     2.97   n=1
    mlp1 fused db1                                4.00e-08  1.36e-08     2.95   n=1
    mlp1 fused dW2                                5.60e-08  3.15e-08     1.78   n=1
    mlp1 fused db2                                1.97e-08  7.02e-09     2.81   n=1
    mlp1 fused dWo                                1.40e-07  5.37e-08     2.61   n=1
    mlp1 fused dbo                                2.03e-05  2.36e-06     8.59   n=65637
    mlp2 fused y                                  2.97e-07  2.42e-07     1.23   n=63
    mlp2 fused g_seg0                             1.46e-07  1.08e-07     1.35   n=64
    mlp2 fused g_seg1                             6.58e-07  4.73e-07     1.39   n=65637
    mlp2 fused g_seg2                             2.59e-07  1.88e-07     1.38   n=257
    mlp2 fused dW1                                3.83e-07  2.00e-07     1.91   n=32
    mlp2 fused db1                                1.82e-05  6.71e-06     2.72   n=65637
    mlp2 fused dW2                                2.38e-07  1.74e-07     1.37   n=32
    mlp2 fused db2                                9.93e-06  4.60e-06     2.16   n=65637
    mlp2 fused dWo                                5.06e-07  2.38e-07     2.13   n=31
    mlp2 fused dbo                                2.24e-05  4.25e-06     5.27   n=65637
    mlp1 fused zero-units y                       3.41e-07  3.85e-07     0.89   n=257
    mlp1 fused zero-units g_seg0                  1.76e-07  1.63e-07     1.08   n=257
    mlp1 fused zero-units g_seg1                  3.79e-07  3.79e-07     1.00   n=257
    mlp1 fused zero-units g_seg2                  1.78e-07  1.40e-07     1.27   n=257
    mlp1 fused zero-units g_seg3                  1.63e-07  1.63e-07     1.00   n=257
    mlp1 fused zero-units g_seg4                  1.71e-07  1.44e-07     1.19   n=257
    mlp1 fused zero-units dW1                     4.15e-07  4.97e-07     0.83   n=257
    mlp1 fused zero-units db1                     3.90e-07  4.32e-07     0.90   n=257
    mlp1 fused zero-units dW2                     3.98e-07  5.62e-07     0.71   n=257
    mlp1 fused zero-units db2                     1.64e-07  1.65e-07     0.99   n=257
    mlp1 fused zero-units dWo                     1.26e-06  2.82e-06     0.45   n=257
    mlp1 fused zero-units dbo                     2.13e-07  4.49e-07     0.47   n=257
    mlp2 fused zero-units y                       4.90e-07  3.71e-07     1.32   n=257
    mlp2 fused zero-units g_seg0                  1.50e-07  1.68e-07     0.89   n=257
    mlp2 fused zero-units g_seg1                  2.35e-07  2.94e-07     0.80   n=257
    mlp2 fused zero-units g_seg2                  1.74e-07  1.22e-07     1.42   n=257
    mlp2 fused zero-units dW1                     7.45e-07  8.22e-07     0.91   n=257
    mlp2 fused zero-units db1                     6.37e-07  4.90e-07     1.30   n=257
    mlp2 fused zero-units dW2                     4.95e-07  7.49e-07     0.66   n=257
    mlp2 fused zero-units db2                     2.51e-07  3.18e-07     0.79   n=257
    mlp2 fused zero-units dWo                     1.43e-06  1.16e-06     1.24   n=257
    mlp2 fused zero-units dbo                     1.89e-07  2.49e-07     0.76   n=257
    mlp1 operand g_x                              4.01e-07  3.59e-07     1.12   n=65637
    mlp1 operand X                                1.19e-07  1.19e-07     1.00   n=63
    mlp1 operand A1                               8.43e-07  8.43e-07     1.00   n=63
    mlp1 operand A2                               1.98e-06  1.98e-06     1.00   n=63
    mlp1 operand G1                               2.22e-07  1.96e-07     1.13   n=65637
    mlp1 operand G2                               9.84e-08  8.91e-08     1.10   n=65637
    mlp1 operand G3                               1.28e-07  1.21e-07     1.06   n=65637
    mlp1 operand dW1                              4.15e-07  3.73e-07     1.11   n=65
    mlp1 operand db1                              1.55e-05  4.79e-06     3.24   n=65637
    mlp1 operand dW2                              1.39e-05  6.93e-06     2.01   n=65637
    mlp1 operand db2                              5.99e-06  3.20e-06     1.87   n=65637
    mlp1 operand dWo                              7.89e-07  6.67e-07     1.18   n=63
    mlp1 operand dbo                              5.98e-06  2.36e-06     2.53   n=65637
    mlp2 operand g_x                              4.63e-07  3.61e-07     1.28   n=65637
    mlp2 operand X                                1.19e-07  1.19e-07     1.00   n=63
    mlp2 operand A1                               9.76e-07  9.76e-07     1.00   n=63
    mlp2 operand A2                               1.41e-06  1.41e-06     1.00   n=63
    mlp2 operand G1                               1.99e-07  1.64e-07     1.22   n=65637
    mlp2 operand G2                               1.15e-07  9.46e-08     1.22   n=65637
    mlp2 operand G3                               1.23e-07  1.14e-07     1.08   n=65637
    mlp2 operand dW1                              5.25e-05  2.20e-05     2.39   n=65637
    mlp2 operand db1                              2.24e-05  6.71e-06     3.34   n=65637
    mlp2 operand dW2                              3.59e-05  1.35e-05     2.66   n=65637
    mlp2 operand db2                              1.12e-05  4.60e-06     2.44   n=65637
    mlp2 operand dWo                              4.47e-07  3.66e-07     1.22   n=65
    mlp2 operand dbo                              1.87e-05  4.25e-06     4.41   n=65637
    sdf fused gE                                  2.30e-07  1.71e-07     1.35   n=31 xyz=0
    sdf fused gG                                  8.80e-08  6.20e-08     1.42   n=31 xyz=0
    sdf fused dW1                                 2.37e-06  2.37e-06     1.00   n=31 xyz=0
    sdf fused db1                                 1.93e-04  7.00e-05     2.76   n=65637 xyz=0
    sdf fused dWo                                 6.30e-05  2.10e-05     3.00   n=65637 xyz=0
    sdf fused dbo                                 9.48e-05  3.04e-05     3.12   n=65637 xyz=1
    sdf fused dWo row 0                           6.30e-05  1.28e-05     4.94   n=65637 xyz=0
    sdf fused J^T gE + 2 g_xyz                    4.29e-07  3.99e-07     1.07   n=31
    sdf operand gE                                2.44e-07  2.44e-07     1.00   n=65
    sdf operand gG                                9.54e-08  9.61e-08     0.99   n=65637
    sdf operand dW1                               3.73e-06  3.97e-06     0.94   n=65
    sdf operand db1                               3.07e-04  7.00e-05     4.39   n=65637
    sdf operand dWo                               5.93e-05  2.10e-05     2.83   n=65637
    sdf operand dbo                               1.65e-04  3.04e-05     5.42   n=65637
    wgrad dW                                      2.35e-04  4.68e-05     5.03   n=65637 M13 N64 gs13 as64
    wgrad db                                      2.82e-04  2.29e-05    12.34   n=65637 M13 N64 gs13 as64
    wgrad dW (db NULL)                            1.83e-04  5.27e-05     3.47   n=65637 M64 N96 gs64 as96
    wgrad dW second call                          6.31e-04  1.14e-04     5.55   n=65637 M64 N64 gs64 as64
    wgrad dW garbage                              7.32e-08  7.28e-08     1.01   n=15 M1 N96 gs4 as96
    wgrad db garbage                              1.59e-04  1.45e-05    10.99   n=65637 M3 N64 gs16 as64
    shade_prep ordinary rows                      6.69e-07  3.52e-07     1.90   n=255 used=ns
    shade_prep clamped rows                       4.31e-03  4.31e-03     1.00   n=255 used=rf
    select_push fwd sdf_grad                      1.16e-07  1.16e-07     1.00   n=257 J=1 used=grad
    select_push g_grad_c                          1.06e-07  1.06e-07     1.00   n=257 J=1 used=grad
    select_push g_out                             2.98e-08  2.98e-08     1.00   n=257 J=1 used=feat+sdf
    select_push g_out column 0                    2.98e-08  2.98e-08     1.00   n=257 J=1 used=feat+sdf
    eikonal sum                                   2.15e-05  6.20e-06     3.46   n=1025
    eikonal grad                                  9.97e-08  1.03e-07     0.96   n=1023
    eikonal partials sum                          2.15e-05  6.20e-06     3.46   n=1025
    eikonal grad via partials (expanded)          9.97e-08  1.03e-07     0.96   n=1023
    eikonal grad via partials (materialised)      9.97e-08  1.03e-07     0.96   n=1023
    alpha alpha                                   3.54e-08  3.12e-08     1.13   beta=1
    alpha g_sdf                                   1.47e-06  1.39e-06     1.06   beta=0.05
    alpha g_beta                                  3.01e-08  3.25e-10    92.62   beta=1
    sh4_bwd                                       5.08e-08  5.08e-08     1.00   n=1 stride=16
    radiance function rgb                         4.04e-07  3.15e-07     1.28   n=257
    radiance function g_feat                      1.94e-07  1.53e-07     1.27   n=257
    radiance function g_refl01                    1.08e-06  6.04e-07     1.79   n=257
    radiance function g_normal                    1.63e-07  1.03e-07     1.58   n=257
    radiance function dW1                         2.89e-07  3.87e-07     0.75   n=257
    radiance function db1                         3.94e-07  4.35e-07     0.91   n=257
    radiance function dW2                         2.89e-07  4.46e-07     0.65   n=257
    radiance function db2                         1.74e-07  2.73e-07     0.64   n=257
    radiance function dWo                         1.41e-06  1.78e-06     0.79   n=257
    radiance function dbo                         1.90e-07  1.90e-07     1.00   n=257
    jac_contract mode 0 v_stride 32               4.51e-07  2.61e-07     1.73   n=257
    jac_contract mode 0 v_stride 68               4.51e-07  2.61e-07     1.73   n=257
    jac_contract mode 1                           1.68e-08  1.68e-08     1.00   n=1
    vi_gather positions                           8.69e-07  8.69e-07     1.00   -
    vi_gather weights                             9.93e-09  9.93e-09     1.00   -
    vi_gather_bwd g_normals                       1.81e-06  3.07e-06     0.59   S=1 missing=None
    vi_gather_bwd g_albedo                        2.93e-06  2.79e-06     1.05   S=1 missing=None
    vi_gather_bwd g_roughness                     1.61e-06  4.12e-06     0.39   S=1 missing=None
    vi_gather_bwd g_metallic                      1.62e-06  1.62e-06     1.00   S=1 missing=None
    vi_gather_bwd g_weights                       5.96e-08  6.53e-08     0.91   S=63 missing=None
    vi_composite rgb                              5.53e-08  5.02e-08     1.10   bg_rays=0
    vi_composite g_w                              5.90e-07  5.90e-07     1.00   bg_rays=0 missing=None
    vi_composite g_Lo                             9.11e-10  9.11e-10     1.00   bg_rays=0 missing=None
    vi_composite g_T                              9.41e-08  9.41e-08     1.00   bg_rays=0 missing=None

The bias gradients (db*) at n = 65 637 are sums that thousands of waves add with float atomics in arbitrary order: their err
moves between runs (wgrad db: 1.0 .. 11.9 x e32 in two runs) and they alone carry the derived random-walk allowance of
tests/backward_refs.py on top of the rule.  alpha g_beta is the one quantity held by the 32-ulp floor rather than by 16 x e32: the twin's sequential fp32 sum of 257 terms
happens to land within 3e-10 of the fp64 value, the kernel's wave-tree sum within 3e-8 (2e-7 of the result).
"""
import ctypes as C
import functools
import itertools

import pytest
import torch

from tests import backward_refs as BR
from tests.backward_refs import compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
N_BIG = BR.N_BIG


@pytest.fixture(scope="module", autouse=True)
def lib():
    from intrinsicavatar_amd import build
    build.build()
    from intrinsicavatar_amd import _lib as L
    yield L.lib()
    print("\n" + "\n".join("TABLE " + r for r in BR.format_table().splitlines()))      # the docstring's table, of this run


def G(t):
    return None if t is None else t.to(DEV).contiguous()


def gpu_empty(*shape):
    return torch.empty(shape, device=DEV)


SENTINEL = 7.0


def guarded(n, cols):
    """an [n, cols] output buffer with one sentinel row behind it (-> check_guard): a store to row n is a ragged-tile bug."""
    full = torch.full((n + 1, cols), SENTINEL, device=DEV)
    return full, full[:n]


def check_guard(what, full):
    assert bool((full[-1] == SENTINEL).all()), f"{what}: the kernel wrote behind the last row"


def assert_zero(what, t):
    assert bool((t == 0).all()), f"{what}: expected exact zeros, max |.| = {float(t.abs().max())}"


def compare_or_zero(what, got, ref64, twin32):
    """the comparison rule; a quantity whose reference is identically zero (a gradient nobody asked for) must be EXACTLY zero."""
    if float(ref64.abs().max()) == 0.0:
        assert_zero(what, got)
    else:
        compare(what, got, ref64, twin32)


# ----------------------------------------------------------------------------------------------------------------------
# ReLU MLPs
@functools.lru_cache(maxsize=None)
def mlp2_case(kind, n, seed, zero=False):
    p = BR.make_mlp2_problem(kind, n, seed, zero_units=zero)
    return p, BR.mlp2_ref(kind, p, F64), BR.mlp2_ref(kind, p, F32)


W_NAMES = ("dW1", "db1", "dW2", "db2", "dWo", "dbo")


def fused_waves(n):
    """waves of a fused backward kernel (32-row tiles, <= 256 workgroups of 4): each adds its bias partial sums with one atomic."""
    return min((n + 31) // 32, 1024)


def wgrad_waves(n):
    """waves of ia_wgrad (16-row slabs, <= 768 workgroups of 4)."""
    return min((n + 15) // 16, 3072)


def bias_adds(name, waves):
    """`atomic_adds` of backward_refs.compare: the bias gradients only."""
    return waves if name.startswith("db") else 0


def run_mlp2_fused(kind, n, seed, zero=False):
    from intrinsicavatar_amd import train_phys
    p, r64, t32 = mlp2_case(kind, n, seed, zero)
    tag = f"mlp{kind} fused n={n}{' zero-units' if zero else ''}"
    segs = [G(s).requires_grad_(True) for s in p["segs"]]
    ws = [G(w).requires_grad_(True) for w in p["weights"]]
    y = train_phys._MLP2.apply(kind, BR.MLP2_OUT[kind], *ws, *segs)
    compare(f"{tag} y", y, r64["y"], t32["y"])
    y.backward(G(p["g_y"]))
    for k, s in enumerate(segs):              # the xyz segment carries the factor 2 of its `mul`
        assert s.grad.shape == p["segs"][k].shape
        compare(f"{tag} g_seg{k}", s.grad, r64["g_segs"][k], t32["g_segs"][k])
    for name, w, a, b in zip(W_NAMES, ws, r64["g_w"], t32["g_w"]):
        compare(f"{tag} {name}", w.grad, a, b, atomic_adds=bias_adds(name, fused_waves(n)))
    return ws


@pytest.mark.parametrize("n", BR.MLP2_NS)
@pytest.mark.parametrize("kind", [1, 2])
def test_mlp2_fused_backward(kind, n):
    """ia_mlp_bwd_fused through train_phys._MLP2 with every segment requiring grad: all segment gradients (every row) and the six
    weight gradients; n around the 32-row tile and past the 256 * 4 * 32 grid cap."""
    run_mlp2_fused(kind, n, BR.MLP2_SEED[(kind, n)])


@pytest.mark.parametrize("kind", [1, 2])
def test_mlp2_fused_backward_exact_zero_preactivations(kind):
    """a unit of each hidden layer whose pre-activation is exactly 0 in every row: torch's ReLU gradient at 0 is 0 and the kernels'
    `v > 0` mask must agree -- nothing may reach that unit's weights."""
    n, seed = BR.MLP2_ZERO_CASE
    ws = run_mlp2_fused(kind, n, seed, zero=True)
    assert_zero("dW1 row 5", ws[0].grad[5]); assert_zero("db1[5]", ws[1].grad[5])
    assert_zero("dW2 row 7", ws[2].grad[7]); assert_zero("db2[7]", ws[3].grad[7])


def _segs_gpu(kind, segs):
    from intrinsicavatar_amd import train
    return train._segs([(s, w, m, a) for s, (w, m, a) in zip(segs, BR.MLP2_SPEC[kind])])


@pytest.mark.parametrize("n", BR.MLP2_OPERAND_NS)
@pytest.mark.parametrize("kind", [1, 2])
def test_mlp2_operand_backward_and_wgrad(lib, kind, n):
    """ia_mlp_bwd (operand path, 64-row tiles) + ia_wgrad: g_x, the emitted layer inputs X / A1 / A2 and pre-activation gradients
    G1 / G2 / G3 against the reference's, then the weight gradients formed from them as train._Radiance.backward does."""
    from intrinsicavatar_amd import _lib as L, train
    p, r64, t32 = mlp2_case(kind, n, BR.MLP2_SEED[(kind, n)])
    tag = f"mlp{kind} operand n={n}"
    IN, OUT = BR.mlp2_in_dim(kind), BR.MLP2_OUT[kind]
    pad = (IN + 1) // 2 * 2
    segs = [G(s) for s in p["segs"]]
    ws = [G(w) for w in p["weights"]]
    ns, ptrs, strides, widths, muls, adds = _segs_gpu(kind, segs)
    fulls, views = zip(*[guarded(n, c) for c in (pad, pad, 64, 64, 64, 64, 16)])
    g_x, X, A1, A2, G1, G2, G3 = views
    L.check(lib.ia_mlp_bwd(L.i32(kind), L.i64(n), L.i32(ns), ptrs, strides, widths, muls, adds, *[L.ptr(w) for w in ws],
                           L.ptr(G(p["g_y"])), L.ptr(g_x), L.i32(pad), L.ptr(X), L.ptr(A1), L.ptr(A2), L.ptr(G1), L.ptr(G2), L.ptr(G3),
                           L.stream()), "ia_mlp_bwd")
    for name, full in zip(("g_x", "X", "A1", "A2", "G1", "G2", "G3"), fulls):
        check_guard(f"{tag} {name}", full)
    compare(f"{tag} g_x", g_x[:, :IN], r64["g_x"], t32["g_x"])
    compare(f"{tag} X", X[:, :IN], r64["X"], t32["X"])
    if pad > IN:
        assert_zero("X pad column", X[:, IN:])
    for name, got in (("A1", A1), ("A2", A2), ("G1", G1), ("G2", G2)):
        compare(f"{tag} {name}", got, r64[name], t32[name])
    compare(f"{tag} G3", G3[:, :OUT], r64["G3"], t32["G3"])
    assert_zero("G3 columns >= OUT", G3[:, OUT:])
    got_w = [*train.wgrad(G1, 64, X, IN), *train.wgrad(G2, 64, A1, 64), *train.wgrad(G3, OUT, A2, 64)]
    for name, got, a, b in zip(W_NAMES, got_w, r64["g_w"], t32["g_w"]):
        compare(f"{tag} {name}", got, a, b, atomic_adds=bias_adds(name, wgrad_waves(n)))


# ----------------------------------------------------------------------------------------------------------------------
# SDF head
@functools.lru_cache(maxsize=None)
def sdf_case(n):
    p = BR.make_sdf_problem(n, BR.SDF_SEED)
    knee, linear = BR.sdf_regime_shares(p)
    assert knee >= 0.5 and linear >= 0.01, (knee, linear)        # the second-order term and the linear softplus branch are exercised
    return p, BR.sdf_ref(p, F64), BR.sdf_ref(p, F32)


def _sdf_args(p):
    from intrinsicavatar_amd import _lib as L, train
    enc, xyz = G(p["enc"]), G(p["xyz"])
    keep = [enc, xyz] + [G(p[k]) for k in ("W1", "b1", "W2", "b2", "jac", "g_out", "q")]
    ns, ptrs, strides, widths, muls, adds = train._segs([(enc, 32, 1.0, 0.0), (xyz, 3, 2.0, -1.0)])
    head = (L.i64(p["n"]), L.i32(ns), ptrs, strides, widths, muls, adds, *[L.ptr(t) for t in keep[2:]])
    return keep, head


@pytest.mark.parametrize("n", BR.SDF_NS)
def test_sdf_fused_backward(lib, n):
    """ia_sdf_mlp_bwd_fused against the DOUBLE BACKWARD of autograd (not the closed form in the kernel's header): gE, gG, the four
    weight gradients (dWo with row 0's second-order term) and g_xyz through d L / d x = J^T gE + 2 g_xyz; both template
    instances (with / without g_xyz) give the same bits for gE / gG."""
    from intrinsicavatar_amd import _lib as L
    p, r64, t32 = sdf_case(n)
    tag = f"sdf fused n={n}"
    keep, head = _sdf_args(p)
    res = {}
    for want_xyz in (False, True):
        (fE, gE), (fG, gG), (fX, g_xyz) = guarded(n, 32), guarded(n, 32), guarded(n, 3)
        d = [torch.zeros(s, device=DEV) for s in ((64, 35), (64,), (13, 64), (13,))]
        if not want_xyz:
            g_xyz = None
        L.check(lib.ia_sdf_mlp_bwd_fused(*head, L.ptr(gE), L.ptr(gG), *[L.ptr(t) for t in d], L.ptr(g_xyz), L.stream()),
                "ia_sdf_mlp_bwd_fused")
        for name, full in (("gE", fE), ("gG", fG), ("g_xyz", fX)):
            check_guard(f"{tag} {name}", full)
        res[want_xyz] = (gE, gG, d, g_xyz)
        t = f"{tag} xyz={int(want_xyz)}"
        compare(f"{t} gE", gE, r64["gE"], t32["gE"])
        compare(f"{t} gG", gG, r64["gG"], t32["gG"])
        for name, got in zip(("dW1", "db1", "dWo", "dbo"), d):
            compare(f"{t} {name}", got, r64[name], t32[name], atomic_adds=bias_adds(name, fused_waves(n)))
        compare(f"{t} dWo row 0", d[2][0], r64["dWo"][0], t32["dWo"][0])
    assert torch.equal(res[False][0], res[True][0]) and torch.equal(res[False][1], res[True][1])
    gE, _, _, g_xyz = res[True]
    total = torch.einsum("nkc,nk->nc", p["jac"].double(), gE.cpu().double()) + 2.0 * g_xyz.cpu().double()
    compare(f"{tag} J^T gE + 2 g_xyz", total, r64["gx"], t32["gx"])


@pytest.mark.parametrize("n", BR.SDF_OPERAND_NS)
def test_sdf_operand_backward_and_wgrad(lib, n):
    """ia_sdf_mlp_bwd (operand path): gE / gG and the weight gradients formed from the operand pairs as train._SDFField.backward
    forms them."""
    from intrinsicavatar_amd import _lib as L, train
    p, r64, t32 = sdf_case(n)
    tag = f"sdf operand n={n}"
    keep, head = _sdf_args(p)
    gE, gG = gpu_empty(n, 32), gpu_empty(n, 32)
    Hh, U = gpu_empty(n, 36), gpu_empty(n, 36)
    DZ, GZ, A, DGS = (gpu_empty(n, 64) for _ in range(4))
    L.check(lib.ia_sdf_mlp_bwd(*head, L.ptr(gE), L.ptr(gG), L.ptr(Hh), L.ptr(U), L.ptr(DZ), L.ptr(GZ), L.ptr(A), L.ptr(DGS),
                               L.stream()), "ia_sdf_mlp_bwd")
    compare(f"{tag} gE", gE, r64["gE"], t32["gE"])
    compare(f"{tag} gG", gG, r64["gG"], t32["gG"])
    dW1, db1 = train.wgrad(DZ, 64, Hh, 35)
    dW1 = dW1 + train.wgrad(GZ, 64, U, 35, want_bias=False)[0]
    dWo, dbo = train.wgrad(keep[7], 13, A, 64)
    dWo[0] += train.wgrad(DGS, 64, DGS, 1)[1]
    for name, got in zip(("dW1", "db1", "dWo", "dbo"), (dW1, db1, dWo, dbo)):
        compare(f"{tag} {name}", got, r64[name], t32[name], atomic_adds=bias_adds(name, wgrad_waves(n)))


# ----------------------------------------------------------------------------------------------------------------------
# split-K weight gradient
def _wgrad_abi(lib, Gm, M, A, N, dW, db):
    from intrinsicavatar_amd import _lib as L
    L.check(lib.ia_wgrad(L.i64(Gm.shape[0]), L.ptr(Gm), L.i32(Gm.stride(0)), L.i32(M), L.ptr(A), L.i32(A.stride(0)), L.i32(N),
                         L.ptr(dW), L.i32(dW.stride(0)), L.ptr(db), L.stream()), "ia_wgrad")


@pytest.mark.parametrize("shape", BR.WGRAD_SHAPES, ids=lambda s: "M{}N{}gs{}as{}".format(*s))
@pytest.mark.parametrize("n", BR.WGRAD_NS)
def test_wgrad(lib, n, shape):
    """ia_wgrad through train.wgrad and the C ABI: db given / NULL, accumulation into the same dW, 1e3 garbage in the columns beyond
    M / N (they only feed discarded accumulator entries), ragged last slab ((13, 64, 13, 64) at n = 17: the scalar tail of the
    slab copy)."""
    from intrinsicavatar_amd import train
    M, N, gs, as_ = shape
    tag = f"wgrad n={n} M{M} N{N} gs{gs} as{as_}"
    alias = shape == (64, 1, 64, 64)
    Gc, Ac = BR.make_wgrad_problem(n, shape, seed=n + M)
    (W64, b64), (W32, b32) = BR.wgrad_ref(Gc, M, Ac, N, F64), BR.wgrad_ref(Gc, M, Ac, N, F32)
    Gg = G(Gc)
    Ag = Gg if alias else G(Ac)
    dW, db = train.wgrad(Gg, M, Ag, N)
    compare(f"{tag} dW", dW, W64, W32)
    compare(f"{tag} db", db, b64, b32, atomic_adds=wgrad_waves(n))
    # db = NULL, then a second call into the same dW: accumulate semantics
    dW1 = torch.zeros((M, N), device=DEV)
    _wgrad_abi(lib, Gg, M, Ag, N, dW1, None)
    compare(f"{tag} dW (db NULL)", dW1, W64, W32)
    dW2 = dW1.clone()
    _wgrad_abi(lib, Gg, M, Ag, N, dW2, None)
    compare(f"{tag} dW second call", dW2, 2.0 * W64, 2.0 * W32.double())
    if n <= 16:                  # a single wave: one atomic per element and call, v + v is exact
        assert torch.equal(dW2, 2.0 * dW1)
    if not alias and (gs > M or as_ > N):
        Gq, Aq = BR.make_wgrad_problem(n, shape, seed=n + M, garbage=1e3)
        dWq, dbq = train.wgrad(G(Gq), M, G(Aq), N)
        compare(f"{tag} dW garbage", dWq, W64, W32)
        compare(f"{tag} db garbage", dbq, b64, b32, atomic_adds=wgrad_waves(n))


# ----------------------------------------------------------------------------------------------------------------------
# shading prep
SUBSETS = [s for s in itertools.product((False, True), repeat=3) if any(s)]


@functools.lru_cache(maxsize=None)
def shade_case(n):
    return BR.make_shade_prep_problem(n, seed=2)


@pytest.mark.parametrize("used", SUBSETS, ids=["+".join(nm for nm, u in zip(("ns", "nw", "rf"), s) if u) for s in SUBSETS])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_shade_prep_backward(n, used):
    """ia_shade_prep_bwd through train._ShadePrep with each non-empty subset of (normal_smpl, normal_world, refl01) as the only
    outputs used (the others reach the kernel as NULL); rows below the 1e-6 clamp of x / max(|x|, 1e-6) -- exact zeros and
    |g| in [1e-9, 1e-7] -- are compared on their own (their gradients are 1e6 times larger), so are the ordinary rows."""
    from intrinsicavatar_amd import train
    p = shade_case(n)
    tag = f"shade_prep n={n} used=" + "+".join(nm for nm, u in zip(("ns", "nw", "rf"), used) if u)
    sg = G(p["sdf_grad"]).requires_grad_(True)
    outs = train._ShadePrep.apply(sg, G(p["rays_d"]), G(p["ray_indices"]), G(p["R"]))
    (sum((G(p["ups"][k]) * outs[k]).sum() for k in range(3) if used[k])).backward()
    r64, _ = BR.shade_prep_ref(p, used, F64)
    t32, _ = BR.shade_prep_ref(p, used, F32)
    small = p["sdf_grad"].double().norm(dim=-1) < 1e-6
    got = sg.grad.cpu()
    compare(f"{tag} ordinary rows", got[~small], r64[~small], t32[~small])
    if bool(small.any()):
        compare(f"{tag} clamped rows", got[small], r64[small], t32[small])


# ----------------------------------------------------------------------------------------------------------------------
# select + push-forward
@pytest.mark.parametrize("n,with_J,used", [(257, True, s) for s in SUBSETS] + [(257, False, (True, True, True)), (1, True, (True, True, True)),
                                                                              (1, False, (True, True, True))])
def test_select_push_forward_and_backward(n, with_J, used):
    """ia_select_push / _bwd through train._SelectPush: invalid rows (defaults 1e5 and (0,0,1), gradient exactly 0), sel = -1 rows,
    fwd_J = None, subsets of used outputs; the sdf gradient adds into column 0 of g_out."""
    from intrinsicavatar_amd import train
    p = BR.make_select_push_problem(n, seed=5)
    tag = f"select_push n={n} J={int(with_J)} used=" + "+".join(nm for nm, u in zip(("feat", "sdf", "grad"), used) if u)
    out, gc = G(p["out"]).requires_grad_(True), G(p["grad_c"]).requires_grad_(True)
    valid = p["valid"]
    feat, sdf, sdf_grad, c2w = train._SelectPush.apply(out, gc, G(valid), G(p["fwd_J"]) if with_J else None, G(p["cand_src"]),
                                                       G(p["sel"]))
    g64o, g64c, f64 = BR.select_push_ref(p, used, with_J, F64)
    g32o, g32c, f32 = BR.select_push_ref(p, used, with_J, F32)
    # forward: copies, masks and the gather are exact; the 3-term dot products of the push-forward follow the rule
    assert torch.equal(feat.cpu(), f32[0]) and torch.equal(sdf.cpu(), f32[1]) and torch.equal(c2w.cpu(), f32[3])
    assert torch.equal(sdf_grad.cpu()[~valid], f32[2][~valid])
    compare_or_zero(f"{tag} fwd sdf_grad", sdf_grad[G(valid)], f64[2][valid], f32[2][valid])
    (sum((G(p["ups"][k]) * o).sum() for k, o in enumerate((feat, sdf, sdf_grad)) if used[k])).backward()
    compare_or_zero(f"{tag} g_out", out.grad, g64o, g32o)
    compare_or_zero(f"{tag} g_grad_c", gc.grad, g64c, g32c)
    assert_zero("g_out on invalid rows", out.grad.cpu()[~valid]); assert_zero("g_grad_c on invalid rows", gc.grad.cpu()[~valid])
    if used[0] and used[1]:
        compare(f"{tag} g_out column 0", out.grad[:, 0], g64o[:, 0], g32o[:, 0])


# ----------------------------------------------------------------------------------------------------------------------
# eikonal term
@pytest.mark.parametrize("n", BR.EIKONAL_NS)
def test_eikonal_forward_and_backward(lib, n):
    """ia_eikonal / _bwd through train._Eikonal and train._EikonalPartials (upstream gradient once as the stride-0 expansion of
    .sum(), once materialised); a zero-norm valid row has gradient 0.  Partials shape: ceil(n / 1024) rows -- except at n = 0,
    where ia_eikonal_partials is 0 and _EikonalPartials returns ONE all-zero row (a sum over it is still 0); both host entries
    return before any launch there, and the gradients are [0, 3]."""
    from intrinsicavatar_amd import train
    p = BR.make_eikonal_problem(n, seed=7)
    w = 0.37
    s64, cnt, g64 = BR.eikonal_ref(p, w, F64)
    s32, _, g32 = BR.eikonal_ref(p, w, F32)
    tag = f"eikonal n={n}"
    sg = G(p["sdf_grad"]).requires_grad_(True)
    valid = G(p["valid"])
    tot, c = train._Eikonal.apply(sg, valid)
    assert float(c) == cnt
    (tot * w).backward()
    assert sg.grad.shape == (n, 3)
    if n == 0:
        assert float(tot) == 0.0
    else:
        compare(f"{tag} sum", tot, s64, s32)
        compare(f"{tag} grad", sg.grad, g64, g32)
        assert_zero("grad on invalid rows", sg.grad.cpu()[~p["valid"]])
    if n > 4:
        assert_zero("grad of the zero-norm row", sg.grad[2])
    k = (n + 1023) // 1024
    assert int(lib.ia_eikonal_partials(n)) == k
    for materialised in (False, True):
        sg2 = G(p["sdf_grad"]).requires_grad_(True)
        part = train._EikonalPartials.apply(sg2, valid)
        assert part.shape == (max(k, 1), 2)
        if n == 0:
            assert_zero("partials at n = 0", part)
        else:
            compare(f"{tag} partials sum", part[:, 0].sum(), s64, s32)
        assert float(part[:, 1].sum()) == cnt
        loss = (part * torch.full(part.shape, w, device=DEV)).sum() if materialised else part.sum() * w
        loss.backward()
        assert sg2.grad.shape == (n, 3)
        if n > 0:
            compare(f"{tag} grad via partials ({'materialised' if materialised else 'expanded'})", sg2.grad, g64, g32)
        assert torch.equal(sg2.grad, sg.grad)


def test_eikonal_all_invalid():
    from intrinsicavatar_amd import train
    p = BR.make_eikonal_problem(1025, seed=7, all_invalid=True)
    sg = G(p["sdf_grad"]).requires_grad_(True)
    tot, c = train._Eikonal.apply(sg, G(p["valid"]))
    (tot * 0.37).backward()
    assert float(tot) == 0.0 and float(c) == 0.0
    assert_zero("grad, all invalid", sg.grad)


# ----------------------------------------------------------------------------------------------------------------------
# Laplace density -> alpha
@pytest.mark.parametrize("beta", [1e-3, 0.05, 1.0])
def test_laplace_alpha_backward(beta):
    """ia_laplace_alpha_bwd through train._Alpha: sdf == 0, +-1e-30, |sdf| / beta = 200 (exp underflows); all gradients finite."""
    from intrinsicavatar_amd import train
    p = BR.make_alpha_problem(257, beta, seed=9)
    tag = f"alpha beta={beta:g}"
    sdf = G(p["sdf"]).requires_grad_(True)
    b = G(p["beta"]).requires_grad_(True)
    a = train._Alpha.apply(sdf, G(p["dists"]), b)
    a.backward(G(p["g_alpha"]))
    gs64, gb64, a64 = BR.alpha_ref(p, F64)
    gs32, gb32, a32 = BR.alpha_ref(p, F32)
    assert bool(torch.isfinite(sdf.grad).all()) and bool(torch.isfinite(b.grad).all())
    compare(f"{tag} alpha", a, a64, a32)
    compare(f"{tag} g_sdf", sdf.grad, gs64, gs32)
    compare(f"{tag} g_beta", b.grad, gb64, gb32)
    assert float(sdf.grad[0]) == 0.0                      # sdf == 0: sign(0) = 0, as in torch


# ----------------------------------------------------------------------------------------------------------------------
# SH4
@pytest.mark.parametrize("g_stride", [16, 68])
@pytest.mark.parametrize("n", [1, 257])
def test_sh4_backward(lib, n, g_stride):
    """ia_sh4_bwd: g_stride 16, and 68 reading columns 48..63 of an [n, 68] buffer whose other columns hold garbage (the view
    train._Radiance.backward passes); corner and centre rows of d01."""
    from intrinsicavatar_amd import _lib as L
    p = BR.make_sh4_problem(n, seed=3)
    if g_stride == 16:
        buf = G(p["g_sh"])
        gp = buf.data_ptr()
    else:
        buf = torch.full((n, 68), 1e3, device=DEV)
        buf[:, 48:64] = G(p["g_sh"])
        gp = buf.data_ptr() + 48 * 4
    out = gpu_empty(n, 3)
    L.check(lib.ia_sh4_bwd(L.i64(n), L.ptr(G(p["d01"])), C.c_void_p(gp), L.i32(g_stride), L.ptr(out), L.stream()), "ia_sh4_bwd")
    compare(f"sh4_bwd n={n} stride={g_stride}", out, BR.sh4_ref(p, F64), BR.sh4_ref(p, F32))


def test_radiance_function_routes_its_gradient_views():
    """train._Radiance.backward end to end past the hash grid: g_feat / g_sh / g_nw are column views of ONE [n, 68] buffer and
    ia_sh4_bwd reads g_sh through its row stride -- a mis-strided view shows in g_refl01.  The hash features the kernel produced
    are an input of the reference; the ReLU repair is backward_refs.make_radiance_problem (2 x the guard band, asserted to cover
    the fp32 SH intermediate; 5 % cap)."""
    from intrinsicavatar_amd import fields, train
    n, seed = BR.RADIANCE_CASE
    table = (torch.randn(fields.hash_n_entries() * 2, generator=BR.seeded(seed + 1)) * 0.3).to(DEV)
    center, scale = torch.full((3,), 0.5), torch.full((3,), 1.25)

    def enc_fn(x):
        xp = ((G(x) - G(center)) / G(scale) + 0.5).contiguous()
        return fields.hashgrid_forward(xp, table).cpu(), xp.cpu()
    p = BR.make_radiance_problem(n, seed, enc_fn)          # asserts the 5 % cap and the coverage of the fp32 SH error
    x = p["x"]
    feat, refl01, nrm = (G(p[k]).requires_grad_(True) for k in ("feat", "refl01", "nrm"))
    ws = [G(w).requires_grad_(True) for w in p["weights"]]
    tg = table.clone().requires_grad_(True)
    rgb = train._Radiance.apply(G(x), tg, feat, refl01, nrm, *ws, G(center), G(scale))
    rgb.backward(G(p["g_rgb"]))
    r64, t32 = BR.radiance_ref(p, F64), BR.radiance_ref(p, F32)
    tag = f"radiance function n={n}"
    compare(f"{tag} rgb", rgb, r64["rgb"], t32["rgb"])
    compare(f"{tag} g_feat", feat.grad, r64["g_feat"], t32["g_feat"])
    compare(f"{tag} g_refl01", refl01.grad, r64["g_refl01"], t32["g_refl01"])
    compare(f"{tag} g_normal", nrm.grad, r64["g_nrm"], t32["g_nrm"])
    for name, w, a, b in zip(W_NAMES, ws, r64["g_w"], t32["g_w"]):
        compare(f"{tag} {name}", w.grad, a, b, atomic_adds=bias_adds(name, fused_waves(n)))
    assert bool(torch.isfinite(tg.grad).all()) and float(tg.grad.abs().max()) > 0


# ----------------------------------------------------------------------------------------------------------------------
# hash-grid Jacobian contractions
@pytest.mark.parametrize("n", [1, 257])
def test_jac_contract(lib, n):
    """ia_hashgrid_jac_contract: mode 0 (J^T v) through train._jac_contract_T with v_stride 32 and 68, mode 1 (J q) through the C ABI."""
    from intrinsicavatar_amd import _lib as L, train
    g = BR.seeded(n)
    jac, v, q = BR.randn(g, n, 32, 3), BR.randn(g, n, 32), BR.randn(g, n, 3)
    jg = G(jac)
    r64, r32 = BR.jac_contract_ref(0, jac, v, F64), BR.jac_contract_ref(0, jac, v, F32)
    compare(f"jac_contract mode 0 n={n} v_stride 32", train._jac_contract_T(jg, G(v)), r64, r32)
    wide = torch.full((n, 68), 1e3, device=DEV)
    wide[:, :32] = G(v)
    compare(f"jac_contract mode 0 n={n} v_stride 68", train._jac_contract_T(jg, wide), r64, r32)
    out = gpu_empty(n, 32)
    L.check(lib.ia_hashgrid_jac_contract(L.i32(1), L.i64(n), L.i32(32), L.ptr(jg), L.ptr(G(q)), L.i32(3), L.ptr(out), L.i32(32),
                                         L.stream()), "ia_hashgrid_jac_contract")
    compare(f"jac_contract mode 1 n={n}", out, BR.jac_contract_ref(1, jac, q, F64), BR.jac_contract_ref(1, jac, q, F32))


# ----------------------------------------------------------------------------------------------------------------------
# volume interaction
def test_vi_gather_forward(lib):
    """ia_vi_gather on a hand-built layout: fg_src / fg_ray / view_dirs and the gathered attributes are pure copies (torch.equal);
    positions o + d t and the re-sampled weights w[s] / count[s] follow the rule.  The foreground list it writes is the one
    ia_vi_gather_bwd's fg_off / fg_counts describe."""
    from intrinsicavatar_amd import _lib as L
    p = BR.make_vi_gather_fwd_problem(seed=4)
    n, Fn = p["n_rays"], p["F"]
    ins = [G(p[k]) for k in ("rpi", "fg_ray_cnt", "fg_start", "ts", "sidx", "fg_cnt", "weights", "rays_o", "rays_d", "normals", "albedo",
                             "rough", "metal")]
    fg_src, fg_ray = torch.full((Fn,), -1, dtype=torch.int32, device=DEV), torch.full((Fn,), -1, dtype=torch.int32, device=DEV)
    pos, view, nrm, alb = (gpu_empty(Fn, 3) for _ in range(4))
    rgh, mtl, rw = (gpu_empty(Fn) for _ in range(3))
    L.check(lib.ia_vi_gather(L.i64(n), *[L.ptr(t) for t in ins], *[L.ptr(t) for t in (fg_src, fg_ray, pos, view, nrm, alb, rgh, mtl, rw)],
                             L.stream()), "ia_vi_gather")
    r64, r32 = BR.vi_gather_fwd_ref(p, F64), BR.vi_gather_fwd_ref(p, F32)
    for name, got in (("fg_src", fg_src), ("fg_ray", fg_ray), ("view_dirs", view), ("normals", nrm), ("albedo", alb), ("rough", rgh),
                      ("metal", mtl)):
        assert torch.equal(got.cpu(), r32[name]), name
    compare("vi_gather positions", pos, r64["positions"], r32["positions"])
    compare("vi_gather weights", rw, r64["weights"], r32["weights"])
    assert torch.equal(fg_src.cpu().long(), torch.repeat_interleave(torch.arange(p["S"]), p["fg_cnt"].long()))


@pytest.mark.parametrize("S", BR.VI_GATHER_SS)
def test_vi_gather_backward(lib, S):
    """ia_vi_gather_bwd with hand-built fg_cnt / fg_off (counts 0 .. 200: some exceed a wave; a block of 64 empty intervals at
    S = 200), all five upstream gradients and each of them NULL in turn; g_weights is the mean over the segment."""
    from intrinsicavatar_amd import _lib as L
    p = BR.make_vi_gather_problem(S, seed=S)
    cnt, off = G(p["cnt"]), G(p["off"])
    ups = [G(u) for u in p["ups"]]
    names = ("g_normals", "g_albedo", "g_roughness", "g_metallic", "g_weights")
    for missing in (None, 0, 1, 2, 3, 4):
        present = [k != missing for k in range(5)]
        outs = [torch.full((S, 3), 9.0, device=DEV), torch.full((S, 3), 9.0, device=DEV)] + [torch.full((S,), 9.0, device=DEV) for _ in range(3)]
        L.check(lib.ia_vi_gather_bwd(L.i64(S), L.ptr(cnt), L.ptr(off), *[L.ptr(u if pr else None) for u, pr in zip(ups, present)],
                                     *[L.ptr(o) for o in outs], L.stream()), "ia_vi_gather_bwd")
        r64, r32 = BR.vi_gather_bwd_ref(p, present, F64), BR.vi_gather_bwd_ref(p, present, F32)
        for k, name in enumerate(names):
            compare_or_zero(f"vi_gather_bwd S={S} missing={missing} {name}", outs[k], r64[k], r32[k])
            assert_zero(f"{name} of empty intervals", outs[k].cpu()[p["cnt"] == 0])


@pytest.mark.parametrize("with_bg_rays", [False, True])
def test_vi_composite_forward_and_backward(lib, with_bg_rays):
    """ia_vi_composite / _bwd on a hand-built layout (70 rays, spp 128): rays without samples (rgb = background, g_T = 0), rays
    with bg_cnt = 0 (T ignored), 1 / 64 / 65 / 128 foreground re-samples; per-ray background given and NULL; each of
    g_w / g_Lo / g_T not requested."""
    from intrinsicavatar_amd import _lib as L
    p = BR.make_vi_composite_problem(seed=4)
    n, Fn = p["n_rays"], p["F"]
    tag = f"vi_composite bg_rays={int(with_bg_rays)}"
    rpi, bgc, frc, fst, fray = (G(p[k]) for k in ("rpi", "bg_cnt", "fg_ray_cnt", "fg_start", "fg_ray"))
    w, Lo, T, bg, g_rgb = (G(p[k]) for k in ("w", "Lo", "T", "bg", "g_rgb"))
    bgr = G(p["bg_rays"]) if with_bg_rays else None
    rgb = gpu_empty(n, 3)
    L.check(lib.ia_vi_composite(L.i64(n), L.ptr(rpi), L.ptr(frc), L.ptr(fst), L.ptr(bgc), L.ptr(w), L.ptr(Lo), L.ptr(T), L.ptr(bg),
                                L.ptr(bgr), L.ptr(rgb), L.stream()), "ia_vi_composite")
    rgb64, gw64, gL64, gT64 = BR.vi_composite_ref(p, with_bg_rays, F64)
    rgb32, gw32, gL32, gT32 = BR.vi_composite_ref(p, with_bg_rays, F32)
    compare(f"{tag} rgb", rgb, rgb64, rgb32)
    empty = p["rpi"][:, 1] == 0
    assert torch.equal(rgb.cpu()[empty], (p["bg_rays"] if with_bg_rays else p["bg"][None].expand(n, 3))[empty])
    for missing in (None, 0, 1, 2):
        g_w = gpu_empty(Fn) if missing != 0 else None
        g_Lo = gpu_empty(Fn, 3) if missing != 1 else None
        g_T = torch.full((n,), 9.0, device=DEV) if missing != 2 else None
        L.check(lib.ia_vi_composite_bwd(L.i64(n), L.i64(Fn), L.ptr(rpi), L.ptr(bgc), L.ptr(fray), L.ptr(w), L.ptr(Lo), L.ptr(bg),
                                        L.ptr(bgr), L.ptr(g_rgb), L.ptr(g_w), L.ptr(g_Lo), L.ptr(g_T), L.stream()),
                "ia_vi_composite_bwd")
        t = f"{tag} missing={missing}"
        if g_w is not None:
            compare(f"{t} g_w", g_w, gw64, gw32)
        if g_Lo is not None:
            compare(f"{t} g_Lo", g_Lo, gL64, gL32)
        if g_T is not None:
            compare(f"{t} g_T", g_T, gT64, gT32)
            assert_zero("g_T of rays without samples / without background", g_T.cpu()[empty | (p["bg_cnt"] == 0)])
