"""CPU checks of tests/forward_refs.py: that the inputs of tests/test_gpu_forward_kernels.py are in the regimes that file claims,
that the autograd reference of the analytic gradient agrees with the closed form, that the level-major helpers are the layout the
kernels document, and that no comparison of the GPU file can fall back to the 32-ulp floor by construction.  Runs anywhere (no
GPU, no library)."""
import pytest
import torch

from tests import backward_refs as BR
from tests import forward_refs as FR

F32, F64 = torch.float32, torch.float64


def _rel(a, b):
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-300)


def _sdf_rows(regime):
    ns = (FR.MLP_NS + FR.VALUE_NS) if regime == "narrow" else (FR.MLP_WIDE_NS + FR.VALUE_WIDE_NS)
    return sorted({FR.problem_rows(n) for n in ns})


# ---- SDF head ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", _sdf_rows("narrow"))
def test_narrow_regime_sits_in_the_softplus_knee(rows):
    """at least half of the (row, unit) pairs with |100 z| < 9.2 and at least 1 % on the pass-through branch 100 z > 20
    (measured at 4099 rows: 0.64 / 0.024 / 0.024 below -20)."""
    knee, above, below, band = FR.sdf_fwd_regime_shares(FR.make_sdf_fwd_problem(rows, "narrow", with_jac=False))
    assert knee >= 0.5 and above >= 0.01, (knee, above, below, band)


@pytest.mark.parametrize("rows", _sdf_rows("wide"))
def test_wide_regime_saturates_both_sides_and_covers_the_branch_boundary(rows):
    """at least a fifth of the pairs on either saturated side and a tenth in 9.2 < |100 z| <= 20, the boundary of softplus100's
    e < 1e-4 branch (measured at 4099 rows: 0.22 knee, 0.28 above 20, 0.27 below -20)."""
    knee, above, below, band = FR.sdf_fwd_regime_shares(FR.make_sdf_fwd_problem(rows, "wide", with_jac=False))
    assert above >= 0.2 and below >= 0.2 and band >= 0.1, (knee, above, below, band)


def test_head_and_value_problems_share_everything_but_the_jacobian():
    a, b = FR.make_sdf_fwd_problem(257, "wide"), FR.make_sdf_fwd_problem(257, "wide", with_jac=False)
    assert all(torch.equal(a[k], b[k]) for k in ("W1", "b1", "W2", "b2", "enc", "x")) and b["jac"] is None
    assert torch.equal(FR.sdf_fwd_ref(a, F64)["out"], FR.sdf_fwd_ref(b, F64)["out"])       # J (x - x.detach()) adds an exact zero
    assert torch.equal(FR.sdf_fwd_ref(a, F32)["out"], FR.sdf_fwd_ref(b, F32)["out"])
    c = FR.make_sdf_fwd_problem(385, "wide")
    assert all(torch.equal(a[k], c[k]) for k in ("W1", "b1", "W2", "b2"))                    # the weights do not depend on the row count


@pytest.mark.parametrize("regime", ["narrow", "wide"])
@pytest.mark.parametrize("rows", [257, 385])
def test_autograd_gradient_matches_the_closed_form(rows, regime):
    """d out[:,0].sum() / d pts by autograd = (J^T g_h[:32] + 2 g_h[32:35]) / s with g_h = (softplus'(z) W2[0]) W1, to 1e-12 of the
    largest entry in fp64.  softplus' is the derivative of Softplus(beta = 100, threshold = 20): sigmoid(100 z) up to the
    threshold, 1 above it -- with the bare sigmoid the two differ by 1 - sigmoid(20) = 2e-9 per saturated unit."""
    p = FR.make_sdf_fwd_problem(rows, regime)
    ref, cf = FR.sdf_fwd_ref(p, F64)["grad"], FR.sdf_fwd_closed_form(p)
    assert _rel(ref, cf) < 1e-12, _rel(ref, cf)
    # each term of the closed form is visible at this precision: without 2 g_h[xyz], or with two extents swapped, it is far off
    z = FR.sdf_preactivation(p)
    sg = torch.where(100.0 * z > 20.0, torch.ones_like(z), torch.sigmoid(100.0 * z))
    gh = (sg * p["W2"].double()[0]) @ p["W1"].double()
    s = torch.tensor(FR.SDF_EXTENT, dtype=F64)
    assert _rel(ref, torch.einsum("nkc,nk->nc", p["jac"].double(), gh[:, :32]) / s) > 1e-3
    assert _rel(ref, cf * s / s[[1, 0, 2]]) > 1e-2


def test_reference_takes_the_value_of_x_from_the_shared_input():
    """the normalisation of pts only carries the derivative 1 / s: out is what the plain formula gives on the fp32 x, in both dtypes."""
    p = FR.make_sdf_fwd_problem(257, "narrow")
    for dt in (F32, F64):
        plain = torch.nn.functional.softplus(FR.sdf_preactivation(p, dt), beta=100) @ p["W2"].to(dt).T + p["b2"].to(dt)
        assert torch.equal(FR.sdf_fwd_ref(p, dt)["out"], plain)


# ---- level-major layouts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 33])
def test_level_major_helpers_round_trip_and_place_every_element(n):
    g = BR.seeded(n)
    enc, jac = BR.randn(g, n, 32), BR.randn(g, n, 32, 3)
    lv, lj = FR.to_levels(enc), FR.to_levels_jac(jac)
    assert lv.shape == (16, n, 2) and lj.shape == (16, n, 6) and lv.is_contiguous() and lj.is_contiguous()
    assert torch.equal(FR.from_levels(lv), enc) and torch.equal(FR.from_levels_jac(lj), jac)
    for l in range(16):
        for f in range(2):
            assert torch.equal(lv[l, :, f], enc[:, 2 * l + f])
            for a in range(3):
                assert torch.equal(lj[l, :, 3 * f + a], jac[:, 2 * l + f, a])
    # the flat float offsets the kernels use: feature 2 l + f of point p at (l n + p) 2 + f, its derivative at (l n + p) 6 + 3 f + a
    p, l, f, a = n - 1, 11, 1, 2
    assert float(lv.reshape(-1)[(l * n + p) * 2 + f]) == float(enc[p, 2 * l + f])
    assert float(lj.reshape(-1)[(l * n + p) * 6 + 3 * f + a]) == float(jac[p, 2 * l + f, a])


# ---- ReLU MLPs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [1, 2])
def test_saturated_problem_reaches_both_ends_of_the_sigmoid(kind):
    """Wo and bo times 40: at least 15 % of the outputs with z3 > 30 and 15 % with z3 < -30 (measured: kind 1 0.21 / 0.51, kind 2
    0.38 / 0.30), the fp32 twin finite; the hidden layers -- and with them the ReLU repair -- are those of the plain problem."""
    n, seed = FR.SATURATED_CASE
    p, r64, t32 = FR.mlp2_case(kind, n, seed, saturated=True)
    z3 = r64["z3"]
    hi, lo = float((z3 > 30).double().mean()), float((z3 < -30).double().mean())
    assert hi >= 0.15 and lo >= 0.15, (hi, lo)
    assert bool(torch.isfinite(t32["y"]).all()) and bool(torch.isfinite(t32["z3"]).all())
    plain = FR.mlp2_problem(kind, n, seed)
    assert all(torch.equal(a, b) for a, b in zip(p["weights"][:4] + p["segs"], plain["weights"][:4] + plain["segs"]))
    assert torch.equal(p["weights"][4], plain["weights"][4] * 40.0) and torch.equal(p["weights"][5], plain["weights"][5] * 40.0)
    assert not bool(BR.mlp2_guard(kind, p["segs"], p["weights"]).any())


@pytest.mark.parametrize("kind", [1, 2])
def test_mlp2_problems_of_every_size_pass_the_relu_repair(kind):
    """make_mlp2_problem asserts its 5 % first-round cap itself; fp32 and fp64 agree on every ReLU sign at every size in use."""
    for rows in sorted({FR.problem_rows(n) for n in FR.MLP_NS}):
        p = FR.mlp2_problem(kind, rows)
        assert p["first_round_redrawn"] <= 0.05 * rows
        f64 = BR.mlp2_forward(kind, BR.up(*p["segs"]), *BR.up(*p["weights"]))
        f32 = BR.mlp2_forward(kind, p["segs"], *p["weights"])
        assert torch.equal(f64["A1"] > 0, f32["A1"] > 0) and torch.equal(f64["A2"] > 0, f32["A2"] > 0)


# ---- no comparison falls back to the floor by construction --------------------------------------------------------------------
def _e32(ref64, twin32):
    return float((twin32.double() - ref64).abs().max())


def test_every_compared_quantity_has_a_positive_fp32_error():
    """e32 > 0 for every (quantity, case) of the GPU file: 16 x e32 is the bar everywhere, never the 32-ulp floor alone."""
    bad = []
    for n, regime in FR.sdf_head_cases():
        _, r64, t32 = FR.sdf_head_case(FR.problem_rows(n), regime)
        bad += [("sdf head", n, regime, k) for k in ("out", "grad") if not _e32(r64[k], t32[k]) > 0]
    for n, regime in FR.sdf_value_cases():
        _, r64, t32 = FR.sdf_value_case(FR.problem_rows(n), regime)
        bad += [("sdf value", n, regime)] if not _e32(r64, t32) > 0 else []
    for kind in (1, 2):
        cases = [(FR.problem_rows(n), FR.MLP2_FWD_SEED, False, False) for n in FR.MLP_NS]
        cases += [(BR.MLP2_ZERO_CASE[0], BR.MLP2_ZERO_CASE[1], True, False), (*FR.SATURATED_CASE, False, True)]
        for c in cases:
            _, r64, t32 = FR.mlp2_case(kind, *c)
            bad += [("mlp2", kind, c)] if not _e32(r64["y"], t32["y"]) > 0 else []
    for n in FR.SH_NS:
        _, r64, t32 = FR.sh_case(FR.problem_rows(n))
        bad += [("sh4", n)] if not _e32(r64, t32) > 0 else []
    assert not bad, bad


def test_sh_problem_holds_the_axis_directions_and_unit_vectors():
    p = FR.make_sh_fwd_problem(257)
    d = p["d01"].double() * 2.0 - 1.0
    assert torch.equal(d[:6], torch.tensor(FR.SH_SPECIAL[:6], dtype=F64))
    assert float((d.norm(dim=-1) - 1.0).abs().max()) < 1e-6
    assert torch.equal(FR.make_sh_fwd_problem(BR.N_BIG)["d01"][:7], p["d01"][:7])


def test_size_constants_are_what_their_derivation_says():
    assert FR.MLP_NS == (1, 31, 32, 33, 63, 65, 383, 384, 385, 98_341)
    assert FR.VALUE_NS == (1, 31, 32, 33, 65, 131_105, 262_177, 393_249, 524_321)
    assert FR.SH_NS == (1, 255, 256, 257, 65_637)
    for k, n in enumerate(FR.VALUE_NS[5:], start=1):
        tiles = (n + 31) // 32
        assert tiles == 4096 * k + 2 and n - (tiles - 1) * 32 == 1             # waves 0 and 1 own k + 1 tiles; the last holds one row
    tiles = (FR.MLP_NS[-1] + 31) // 32
    assert tiles == 3072 + 2 and FR.MLP_NS[-1] - (tiles - 1) * 32 == 5


def test_compare_rows_is_backward_refs_compare_on_whole_problems_and_uses_all_rows_for_a_prefix():
    g = BR.seeded(0)
    ref = BR.randn(g, 257, 3).double()
    twin = ref + 1e-5 * BR.randn(g, 257, 3).double()                              # 16 e32 well above the 32-ulp floor
    e32 = float((twin - ref).abs().max())
    assert 15.0 * e32 > BR.FLOOR_ULPS * 2.0 ** -23 * float(ref.abs().max())
    n0 = len(BR.TABLE)
    FR.compare_rows("whole", ref + 15.0 * e32, ref, twin)
    BR.compare("whole", ref + 15.0 * e32, ref, twin)
    assert BR.TABLE[n0][1:] == BR.TABLE[n0 + 1][1:]
    FR.compare_rows("prefix", ref[:1] + 15.0 * e32, ref, twin)                  # the bar of a one-row prefix is the problem's
    with pytest.raises(AssertionError):
        FR.compare_rows("prefix", ref[:1] + 17.0 * e32, ref, twin)
    with pytest.raises(AssertionError):
        FR.compare_rows("shape", ref[:1, :2], ref, twin)
    del BR.TABLE[n0:]
