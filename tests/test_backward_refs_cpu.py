"""CPU checks of tests/backward_refs.py: the references and input generators that tests/test_gpu_backward_kernels.py compares
the training-backward kernels with.  Runs anywhere (no GPU, no library)."""
import numpy as np
import pytest
import torch

from tests import backward_refs as BR


def _rel(a, b):
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-300)


# ---- SDF head -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 33, 257])
def test_sdf_double_backward_matches_the_closed_form(n):
    """the autograd (double backward) reference against the closed form the kernels were derived from, as a second opinion."""
    p = BR.make_sdf_problem(n, seed=11)
    ref, cf = BR.sdf_ref(p, torch.float64), BR.sdf_closed_form(p)
    for k in ("gE", "gG", "dW1", "db1", "dWo", "dbo", "gx"):
        assert _rel(ref[k], cf[k]) < 1e-7, (k, _rel(ref[k], cf[k]))
    # the pairing ia_hashgrid_bwd relies on: d L / d J = gG (x) q
    pair = ref["gG"][:, :, None] * p["q"].double()[:, None, :]
    assert _rel(ref["gJ"], pair) < 1e-12
    # d L / d x = J^T gE + 2 g_xyz
    total = torch.einsum("nkc,nk->nc", p["jac"].double(), ref["gE"]) + 2.0 * cf["g_xyz"]
    assert _rel(ref["gx"], total) < 1e-7


@pytest.mark.parametrize("n", sorted(set(BR.SDF_NS + BR.SDF_OPERAND_NS)))
def test_sdf_inputs_exercise_the_softplus_knee_and_the_linear_branch(n):
    """at least half of the (row, unit) pairs inside |100 z| < 10, at least 1 % on the linear branch 100 z > 20 (64 units: the
    shares are meaningful for a single row too)."""
    knee, linear = BR.sdf_regime_shares(BR.make_sdf_problem(n, BR.SDF_SEED))
    assert knee >= 0.5 and linear >= 0.01, (knee, linear)


# ---- ReLU MLPs -----------------------------------------------------------------------------------------------------------
def _mlp2_cases():
    cases = [(k, n, BR.MLP2_SEED[(k, n)], False) for k in (1, 2) for n in BR.MLP2_NS]
    cases += [(k, BR.MLP2_ZERO_CASE[0], BR.MLP2_ZERO_CASE[1], True) for k in (1, 2)]
    return cases


@pytest.mark.parametrize("kind,n,seed,zero", _mlp2_cases())
def test_relu_generator_leaves_no_row_in_the_guard_band(kind, n, seed, zero):
    """make_mlp2_problem asserts the 5 % first-round cap itself; here: nothing is left inside the band, fp32 and fp64 agree on
    every ReLU sign, and their gradients are as close as fp32 allows."""
    p = BR.make_mlp2_problem(kind, n, seed, zero_units=zero)
    assert p["first_round_redrawn"] <= 0.05 * n
    assert not bool(BR.mlp2_guard(kind, p["segs"], p["weights"]).any())
    r64, t32 = BR.mlp2_ref(kind, p, torch.float64), BR.mlp2_ref(kind, p, torch.float32)
    assert torch.equal(r64["A1"] > 0, t32["A1"] > 0) and torch.equal(r64["A2"] > 0, t32["A2"] > 0)
    assert _rel(t32["g_x"].double(), r64["g_x"]) < 1e-5
    if zero:
        assert bool((r64["A1"][:, 5] == 0).all()) and bool((r64["A2"][:, 7] == 0).all())
        assert bool((r64["G1"][:, 5] == 0).all()) and bool((r64["G2"][:, 7] == 0).all())
        assert bool((r64["g_w"][0][5] == 0).all()) and bool((r64["g_w"][2][7] == 0).all())


def test_relu_generator_is_deterministic():
    a, b = BR.make_mlp2_problem(1, 257, 1), BR.make_mlp2_problem(1, 257, 1)
    assert all(torch.equal(x, y) for x, y in zip(a["segs"] + a["weights"], b["segs"] + b["weights"]))


# ---- SH4 -------------------------------------------------------------------------------------------------------------------
def test_sh4_closed_form_matches_the_oracle(oracle):
    """the same directions as tests/test_gpu_fields.py::test_sh4_vs_oracle_and_closed_form."""
    rng = np.random.default_rng(5)
    d = rng.normal(size=(4096, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d01 = (d + 1) / 2
    out = BR.sh4(torch.from_numpy(d01).double()).numpy()
    np.testing.assert_allclose(out, oracle.sh4(d01), rtol=1e-5, atol=1e-6)
    G = out.T @ out / d.shape[0] * 4 * np.pi
    assert np.abs(G - np.eye(16)).max() < 0.15


# ---- the small generators: the edges the GPU file relies on are really there ---------------------------------------------
def test_shade_prep_inputs_hold_the_clamped_and_zero_rows():
    p = BR.make_shade_prep_problem(257, seed=2)
    nrm = p["sdf_grad"].double().norm(dim=-1)
    assert int((nrm == 0).sum()) >= 8
    tiny = (nrm > 0) & (nrm < 1e-6)
    assert int(tiny.sum()) >= 8 and bool(((nrm[tiny] >= 0.99e-9) & (nrm[tiny] <= 1.01e-7)).all())
    assert bool((nrm[(nrm > 0) & ~tiny] >= 1e-3).all())
    ri = p["ray_indices"]
    assert bool((ri[1:] < ri[:-1]).any()) and ri.unique().numel() < ri.numel()
    g64, _ = BR.shade_prep_ref(p, (True, True, True), torch.float64)
    assert bool(torch.isfinite(g64).all())


def test_vi_layouts_are_consistent():
    for S in BR.VI_GATHER_SS:
        p = BR.make_vi_gather_problem(S, seed=S)
        assert int(p["cnt"].max()) > 64 or S > 1 and int(p["cnt"][0]) == 65
        assert torch.equal(p["off"].long(), torch.cumsum(p["cnt"].long(), 0) - p["cnt"].long())
    p = BR.make_vi_gather_problem(200, seed=200)
    assert bool((p["cnt"][64:128] == 0).all())
    c = BR.make_vi_composite_problem(seed=4)
    has = c["rpi"][:, 1] > 0
    assert bool((c["rpi"][has, 1] == c["spp"]).all()) and bool((c["fg_ray_cnt"][~has] == 0).all())
    assert bool((c["fg_ray_cnt"][has] + c["bg_cnt"][has] == c["spp"]).all())
    assert set([0, 1, 64, 65, 128]) <= set(c["fg_ray_cnt"][has].tolist()) and bool((~has).any())
    assert int(c["fg_ray"].shape[0]) == c["F"] == int(c["fg_ray_cnt"].sum())


def test_radiance_generator_cap_and_sh_coverage():
    """make_radiance_problem asserts its own 5 % first-round cap and that the widened band covers the fp32 SH error; here with a
    stand-in for the hash features of the magnitude the GPU test's table (randn * 0.3) gives."""
    n, seed = BR.RADIANCE_CASE
    p = BR.make_radiance_problem(n, seed, lambda x: (BR.randn(BR.seeded(5), n, 32), x))
    assert p["first_round_redrawn"] <= 0.05 * n
    sh = BR.sh4(p["refl01"].double()).float()
    assert not bool(BR.mlp2_guard(1, [p["enc"], p["xp"], p["feat"], sh, p["nrm"]], p["weights"], margin=BR.RADIANCE_MARGIN).any())


def test_vi_gather_forward_layout_is_the_one_the_backward_reads():
    p = BR.make_vi_gather_fwd_problem(seed=4)
    r = BR.vi_gather_fwd_ref(p, torch.float64)
    assert torch.equal(r["fg_src"].long(), torch.repeat_interleave(torch.arange(p["S"]), p["fg_cnt"].long()))
    assert torch.equal(p["fg_off"].long(), torch.cumsum(p["fg_cnt"].long(), 0) - p["fg_cnt"].long())
    assert int(p["fg_cnt"].sum()) == p["F"] and bool((p["fg_cnt"] == 0).any()) and int(p["fg_cnt"].max()) > 64
    for r_ in range(p["n_rays"]):                                  # foreground re-samples name their intervals in non-decreasing order
        b, nf = int(p["rpi"][r_, 0]), int(p["fg_ray_cnt"][r_])
        assert bool((p["sidx"][b + 1:b + nf] >= p["sidx"][b:b + nf - 1]).all())


def test_table_folding_keeps_the_worst_case_of_each_quantity():
    rows = [("mlp1 fused n=1 y", 1.0, 0.5, 2.0), ("mlp1 fused n=65637 y", 3.0, 1.0, 3.0), ("wgrad n=17 M13 N64 gs13 as64 dW", 1.0, 1.0, 1.0),
            ("shade_prep n=255 used=ns+rf clamped rows", 2.0, 1.0, 2.0), ("plain", 1.0, 1.0, 1.0)]
    assert BR.fold_table(rows) == [("mlp1 fused y", 3.0, 1.0, 3.0, "n=65637"), ("wgrad dW", 1.0, 1.0, 1.0, "n=17 M13 N64 gs13 as64"),
                                   ("shade_prep clamped rows", 2.0, 1.0, 2.0, "n=255 used=ns+rf"), ("plain", 1.0, 1.0, 1.0, "-")]
    assert len(BR.format_table(rows).splitlines()) == 5


def test_compare_rule():
    ref = torch.tensor([1.0, -2.0], dtype=torch.float64)
    twin = ref + torch.tensor([1e-7, 0.0], dtype=torch.float64)
    BR.compare("ok", ref + 1.5e-6, ref, twin)
    with pytest.raises(AssertionError):
        BR.compare("too far", ref + 8e-6, ref, twin)
    with pytest.raises(AssertionError):
        BR.compare("vacuous", ref * 0, ref * 0, ref * 0)
    BR.compare("floor", ref + 5e-6, ref, ref)                 # twin exact: the 32-ulp floor (7.6e-6 here) applies
