"""CPU: the reference of the hash-grid table backward (tests/hash_bwd_refs.py) checked before the GPU tests lean on it.

  layout     make_cfg restated in Python equals oracle.hashgrid_offsets (offsets, resolutions, fp32 scales bit for bit)
  (a)        the oracle's fp32 first-order backward and its forward (enc, J) agree with the reference PER LEVEL by the rule of
             tests/backward_refs.py (the oracle as `got`), points outside the cube included: this ties the index function
  (b)        the fp64 reference equals fp64 torch autograd, with respect to the table, of <gE, enc> + <gG, J q> built from the
             forward reference, to 1e-12 of the largest entry -- first- and second-order term, every corner class and axis
  (c)        the generator conditions hold for the committed seeds
"""
import numpy as np
import pytest
import torch

from tests import hash_bwd_refs as HR
from tests.backward_refs import compare

F32, F64 = torch.float32, torch.float64
CONFIG_NAMES = tuple(HR.CONFIGS)


def oracle_layout(oracle, c):
    total, offs, res, sc = oracle.hashgrid_offsets(c)
    return total, [int(o) for o in offs], [int(r) for r in res], [float(s) for s in sc]


@pytest.mark.parametrize("name", CONFIG_NAMES + ("over64",))
def test_layout_restates_make_cfg(oracle, name):
    c = HR.OVER_64_SLICES if name == "over64" else HR.cfg(name)
    assert HR.layout(c) == oracle_layout(oracle, c)
    if name == "over64":
        assert HR.n_slices(HR.layout(c)) == [1, 2, 5, 15, 44, 128, 128, 128]           # 451 buckets, three levels past 64 slices
    else:
        assert max(HR.n_slices(HR.layout(c))) <= 64
    if name == "odd5":
        _, offs, res, _ = HR.layout(c)
        sizes = [offs[l + 1] - offs[l] for l in range(5)]
        assert all(s & (s - 1) for s in sizes[1:]) and all(r ** 3 <= s for r, s in zip(res, sizes))      # dense, no power of two
    if name == "small12":
        _, offs, res, _ = HR.layout(c)
        assert all(offs[l + 1] - offs[l] == 4096 for l in range(6)) and all(r ** 3 > 4096 for r in res[1:])    # hashed from level 1


def _points(guarded):
    """uniform, outside the cube, far outside, and the special points"""
    xs = [HR.make_points(kind, n, seed, guarded)[0] for kind, n, seed in (("uniform", 1500, 11), ("near", 1000, 16), ("far", 100, 17),
                                                                          ("special", 8, 15))]
    return torch.cat(xs)


@pytest.mark.parametrize("name", CONFIG_NAMES)
def test_first_order_reference_against_the_oracle_per_level(oracle, name):
    c = HR.cfg(name)
    lay = oracle_layout(oracle, c)
    L = c["n_levels"]
    x = _points(False)
    g = torch.randn(x.shape[0], 2 * L, generator=torch.Generator().manual_seed(3))
    got = torch.from_numpy(oracle.hashgrid_bwd_params(x.numpy(), g.numpy(), lay[0] * 2, c))
    r64, r32 = HR.table_grad(x, g, None, None, lay, F64), HR.table_grad(x, g, None, None, lay, F32)
    for l, sl in HR.level_slices(lay):
        compare(f"oracle bwd {name} level={l}", got[sl], r64[sl], r32[sl])


@pytest.mark.parametrize("name", CONFIG_NAMES)
def test_forward_reference_against_the_oracle_per_level(oracle, name):
    c = HR.cfg(name)
    lay = oracle_layout(oracle, c)
    x = _points(True)                        # J is discontinuous across a lattice plane: guarded points
    params = (torch.rand(lay[0] * 2, generator=torch.Generator().manual_seed(5)) * 0.2 - 0.1)
    enc, jac = oracle.hashgrid_fwd(x.numpy(), params.numpy(), c, with_jac=True)
    e64, j64 = HR.forward(x, params, lay, F64)
    e32, j32 = HR.forward(x, params, lay, F32)
    for l in range(c["n_levels"]):
        k = slice(2 * l, 2 * l + 2)
        compare(f"oracle fwd enc {name} level={l}", torch.from_numpy(enc)[:, k], e64[:, k], e32[:, k])
        compare(f"oracle fwd J {name} level={l}", torch.from_numpy(jac)[:, k], j64[:, k], j32[:, k])


@pytest.mark.parametrize("mode", HR.MODES)
@pytest.mark.parametrize("name", CONFIG_NAMES)
def test_reference_equals_fp64_autograd(name, mode):
    c = HR.cfg(name)
    lay = HR.layout(c)
    L = c["n_levels"]
    x = _points(True)[::5]
    g = torch.Generator().manual_seed(9)
    n = x.shape[0]
    gE = torch.randn(n, 2 * L, generator=g, dtype=F64) if mode != "second" else None
    gG = torch.randn(n, 2 * L, generator=g, dtype=F64) if mode != "first" else None
    q = torch.randn(n, 3, generator=g, dtype=F64) if mode != "first" else None
    params = torch.zeros(lay[0] * 2, dtype=F64, requires_grad=True)
    enc, jac = HR.forward(x, params, lay, F64)
    loss = 0.0
    if gE is not None:
        loss = loss + (gE * enc).sum()
    if gG is not None:
        loss = loss + (gG * torch.einsum("nkc,nc->nk", jac, q)).sum()
    auto, = torch.autograd.grad(loss, params)
    ref = HR.table_grad(x, gE, gG, q, lay, F64)
    for l, sl in HR.level_slices(lay):
        scale = float(auto[sl].abs().max())
        assert scale > 0.0
        assert float((ref[sl] - auto[sl]).abs().max()) <= 1e-12 * scale, (name, mode, l)


@pytest.mark.parametrize("kind,n,seed,guard_levels", HR.POINT_SETS)
def test_generator_conditions(kind, n, seed, guard_levels):
    x, first = HR.make_points(kind, n, seed, True, guard_levels)
    raw, _ = HR.make_points(kind, n, seed, False)
    assert x.shape == (n, 3) and x.dtype == F32
    assert int(HR.near_lattice(x, HR.guard_scales(guard_levels)).sum()) == 0      # none remains
    if kind == "uniform" and guard_levels == 16:
        assert 0.005 * n < first < 0.03 * n, first                                # 1.3 % of uniform points under configuration A
        assert int((x != raw).any(-1).sum()) == first                             # re-drawn, and only those
    if kind == "same":
        assert bool((x == x[0]).all())
    if kind == "alt2":
        assert bool((x[0::2] == x[0]).all()) and bool((x[1::2] == x[1]).all()) and bool((x[0] != x[1]).any())
    if kind == "special":
        assert bool((raw[2] == 0.5).all()) and int(HR.near_lattice(raw, HR.guard_scales()).sum()) >= 1     # the centre IS a lattice point
    if kind == "near":
        assert bool((raw < 0).any()) and bool((raw > 1).any())
    if kind == "far":
        assert float(raw.abs().max()) > 15.0


def test_split_bucket_sizes():
    """the two large cases of the GPU file are what they are there for: two parts on level 0 of A, more than 64 parts' worth on `one`"""
    part, max_parts = 1 << 19, 64
    assert part < HR.N_TWO_PARTS * 8 <= 2 * part
    assert HR.N_CLAMPED_PARTS * 8 > max_parts * part and HR.N_CLAMPED_PARTS * 8 < 2 ** 31
    assert HR.N_FULL * 8 <= part                                     # a single part per bucket: bit-reproducible reduce
    assert HR.N_GUARD_CASE >= 1 << 15


def test_problem_modes():
    p = HR.make_problem("special", 8, 15)
    x, gE, gG, q = HR.mode_inputs(p, "first", n_levels=5)
    assert gG is None and q is None and gE.shape == (8, 10) and bool((x[2] == 0.5).all())
    x, gE, gG, q = HR.mode_inputs(p, "second", 3, n_levels=1)
    assert gE is None and gG.shape == (3, 2) and q.shape == (3, 3) and x.shape == (3, 3)
    assert np.isfinite(p["gE"].numpy()).all()
