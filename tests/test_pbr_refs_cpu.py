"""CPU checks of tests/pbr_refs.py: the references and the per-class input generator that tests/test_gpu_pbr_kernels.py compares the PBR
shading kernels with.  Runs anywhere (no GPU, no library)."""
import functools

import pytest
import torch

from tests import pbr_refs as PR

F32, F64 = torch.float32, torch.float64
BIG = 1 << 18
# every (F, map) the GPU module runs
SMALL_CASES = [(F, hw) for F in (1, 255, 256, 257) for hw in ((5, 7), (16, 32))]
BIG_CASES = [(BIG - 1, (24, 512)), (BIG, (24, 512)), (BIG + 8192 + 1, (24, 512)), (BIG, (256, 512))]
DECISIONS = ("x0", "x1", "y0", "y1", "flag", "pdf_y", "pdf_x", "masked", "need_env", "lit", "front", "pdf_zero", "pdf_branch", "mis_on")


@functools.lru_cache(maxsize=4)
def problem(F, hw, indirect=True):
    return PR.make_problem(F, hw, seed=1, indirect=indirect)


@pytest.mark.parametrize("hw", PR.MAPS)
def test_constructed_directions_keep_their_distance_from_every_texel_boundary(hw):
    """2^18 directions per map: fp32 and fp64 take the same bilinear footprint and the same pdf texel for EVERY direction, the smallest
    distance to a boundary stays >= 0.0997 texel (0.01 for the one fixed direction of the NoL == 0 class), seam and clamped rows occur."""
    H, W = hw
    p = problem(BIG, hw)
    d64 = p["wo"].double() @ p["R"].double()
    d32 = p["wo"] @ p["R"]
    d64, d32 = d64 / d64.norm(dim=-1, keepdim=True), d32 / d32.norm(dim=-1, keepdim=True)
    a, b = PR.footprint(d64, H, W), PR.footprint(d32, H, W)
    for k in ("x0", "x1", "y0", "y1", "flag"):
        assert torch.equal(a[k], b[k]), k
    assert all(torch.equal(s, t) for s, t in zip(PR.pdf_texel(d64, H, W), PR.pdf_texel(d32, H, W)))
    dist = torch.minimum(PR.boundary_distance(d64, H, W), PR.boundary_distance(d32.double(), H, W))
    zero = PR.mask_of(p["lab"]["cos"], "nol_zero")
    assert float(dist[~zero].min()) >= 0.0997, float(dist[~zero].min())
    assert float(dist[zero].min()) >= 0.01
    assert int(((a["x0"] == W - 1) & (a["x1"] == 0)).sum()) >= PR.MIN_ROWS
    assert int((a["flag"] & (a["y0"] == 0)).sum()) >= PR.MIN_ROWS and int((a["flag"] & (a["y0"] == H - 1)).sum()) >= PR.MIN_ROWS


@pytest.mark.parametrize("F,hw", SMALL_CASES + BIG_CASES)
def test_every_class_is_populated_and_is_what_its_name_says(F, hw):
    H, W = hw
    p = problem(F, hw)
    lab = p["lab"]
    tables = dict(cos=PR.COS, tr=PR.TRS, texel=PR.TEXEL, rough=PR.ROUGH, metal=PR.METAL, albedo=PR.ALBEDO)
    if F >= 257:
        for k, tab in tables.items():
            for name in set(tab):
                assert lab[k].count(name) >= PR.MIN_ROWS, (k, name, lab[k].count(name))
    tail = F % 256
    if tail >= 56:            # 56 rows = 7 values of i // 8: every value of every attribute (F = 257 has one such row: see shift_for)
        for k, tab in tables.items():
            assert lab[k].values(F - tail) == set(tab), k
    r = PR.shade_ref(p, "light", F64, used=(False, False, False))["dec"]
    is_ = lambda k, *v: PR.mask_of(lab[k], *v)      # noqa: E731
    n, wo, wi = p["n"], p["wo"], -p["view_dirs"]
    for dt in (F32, F64):
        NoL, NoV = (n.to(dt) * wo.to(dt)).sum(-1), (n.to(dt) * wi.to(dt)).sum(-1)
        assert bool((NoL[is_("cos", "nol_zero")] == 0).all())
        assert bool((NoL[is_("cos", "nol_neg")] <= -0.0199).all()) and bool((NoL[is_("cos", "front", "nov_neg")] >= 0.0199).all())
        assert bool((NoV[is_("cos", "nov_neg")] <= -0.0199).all()) and bool((NoV[~is_("cos", "nov_neg")] >= 0.0199).all())
        assert bool(((NoL + NoV).abs() >= 0.0199).all())
        # the pdf branch of mis / mats (NoH > 0 && VoH > 0): NoH = (NoL + NoV) / |wi + wo| as above, VoH = |wi + wo| / 2 for every row
        h = wi.to(dt) + wo.to(dt)
        hl = h.norm(dim=-1)
        assert bool((hl >= 0.1).all()) and bool((((wi.to(dt) * h).sum(-1) / hl) >= 0.05).all())
    for name, val in PR.TR_VALUE.items():
        assert bool((p["tr"][is_("tr", name)] == torch.tensor(val)).all())
    inner = p["tr"][is_("tr", "interior")]
    assert bool(((inner > 0) & (inner < 1)).all())
    for name, val in PR.ROUGH_VALUE.items():
        assert bool((p["rough"][is_("rough", name)] == torch.tensor(val)).all())
    assert bool((p["metal"][is_("metal", "zero")] == 0).all()) and bool((p["metal"][is_("metal", "one")] == 1).all())
    assert bool((p["albedo"][is_("albedo", "c0_zero"), 0] == 0).all()) and bool((p["albedo"][is_("albedo", "c0_one"), 0] == 1).all())
    m = is_("albedo", "c2_zero_c1_one")
    assert bool((p["albedo"][m, 2] == 0).all()) and bool((p["albedo"][m, 1] == 1).all())
    # texel classes (the NoL == 0 rows have their one fixed direction instead)
    geo = ~is_("cos", "nol_zero")
    s = is_("texel", "seam") & geo
    assert bool(((r["x0"] == W - 1) & (r["x1"] == 0))[s].all())
    t, b = is_("texel", "top") & geo, is_("texel", "bottom") & geo
    assert bool((r["flag"] & (r["y0"] == 0))[t].all()) and bool((r["flag"] & (r["y0"] == H - 1))[b].all())
    i = is_("texel", "interior") & geo
    assert bool((~r["flag"] & (r["x1"] == r["x0"] + 1))[i].all())
    z = is_("texel", "zero_pmf") & geo
    assert bool(((r["pdf_y"] == p["target"][:, 0]) & (r["pdf_x"] == p["target"][:, 1]))[z].all())
    assert bool((p["pmf"][r["pdf_y"], r["pdf_x"]][z] == 0).all()) and bool((p["pmf"].flatten() == 0).sum() == len(PR.zero_texels(H, W)))
    # (a direction of another class may have a zero texel as its nearest too)
    assert bool((r["pdf_zero"] == ((p["pmf"][r["pdf_y"], r["pdf_x"]] == 0) & r["need_env"])).all()) and bool(r["pdf_zero"][z & r["need_env"]].all())
    if F >= 257:
        # rows where the class is at work: lit, with a live environment lookup (tr > 0 after the clamp)
        for name in PR.TEXEL:
            assert int((is_("texel", name) & r["need_env"]).sum()) >= PR.MIN_ROWS // 2, name
        assert int((is_("tr", "zero", "below") & ~r["masked"]).sum()) >= PR.MIN_ROWS
        assert int((is_("cos", "nov_neg") & r["lit"] & ~r["front"]).sum()) >= PR.MIN_ROWS
    if F >= BIG and H == 24:
        # default record path: bands of TH64 = 11 rows; y0 = 10 and 21 have their y1 neighbour in the next band's first row
        for y0 in (0, 10, 21, 23):
            assert int(((r["y0"] == y0) & r["need_env"]).sum()) >= PR.MIN_ROWS, y0


@pytest.mark.parametrize("mode", list(PR.MODES))
@pytest.mark.parametrize("indirect", [False, True])
@pytest.mark.parametrize("F,hw", [(257, (5, 7)), (257, (16, 32)), (1, (16, 32))])
def test_fp32_and_fp64_take_the_same_decisions_and_masked_rows_are_exactly_zero(mode, indirect, F, hw):
    p = problem(F, hw, indirect)
    r64, t32 = PR.shade_ref(p, mode, F64), PR.shade_ref(p, mode, F32)
    for k in DECISIONS:
        assert torch.equal(r64["dec"][k], t32["dec"][k]), k
    masked = r64["dec"]["masked"]
    dark = masked | ~r64["dec"]["lit"]                       # mis / mats have no cosine mask, their unlit rows are zero by the BRDF
    for r in (r64, t32):
        for k in ("Lo", "Lo_diff", "Lo_spec"):
            assert bool((r[k][dark] == 0).all()), k
        if PR.MODES[mode] <= 1:
            for k in ("g_normal", "g_albedo", "g_roughness", "g_metallic"):
                assert bool((r[k][masked] == 0).all()), k
                assert bool(torch.isfinite(r[k]).all())
                if F > 1:
                    assert float(r[k].abs().max()) > 0, k
            back = PR.mask_of(p["lab"]["cos"], "nov_neg")
            assert bool((r["g_roughness"][back] == 0).all())          # specular off, diffuse on
            if F > 1:
                assert float(r["g_env"].abs().max()) > 0 and float(r["g_normal"][back & ~masked].abs().max()) > 0
    if PR.MODES[mode] <= 1 and F > 1:
        for used in ((True, False, False), (False, True, False), (False, False, True)):
            r = PR.shade_ref(p, mode, F64, used=used)
            for k in ("g_normal", "g_albedo", "g_roughness", "g_metallic", "g_env"):
                if k in ("g_albedo", "g_metallic", "g_roughness") and used[1]:
                    continue            # Lo_diff does not depend on the material
                assert float(r[k].abs().max()) > 0, (used, k)
        r = PR.shade_ref(p, mode, F64, used=(False, True, False))
        for k in ("g_albedo", "g_roughness", "g_metallic"):
            assert float(r[k].abs().max()) == 0


@pytest.mark.parametrize("F,hw", BIG_CASES)
def test_big_batches_agree_on_every_decision(F, hw):
    p = problem(F, hw)
    for mode in ("light", "uniform_light"):
        a, b = PR.shade_ref(p, mode, F64, used=(False,) * 3)["dec"], PR.shade_ref(p, mode, F32, used=(False,) * 3)["dec"]
        for k in DECISIONS:
            assert torch.equal(a[k], b[k]), (mode, k)
    assert PR.texel_adds(a, hw) >= 4


@pytest.mark.parametrize("mode", ["light", "uniform_light"])
def test_fp64_autograd_agrees_with_central_differences_of_the_forward(mode):
    """guards the reference itself: every per-point gradient of every ordinary row (front-facing, lit, mid roughness) against
    (L(x + h) - L(x - h)) / 2h of the fp64 forward, and the gradient of a handful of texels likewise.  h = 1e-6: the truncation term
    h^2 f''' / 6 and the rounding term 2^-53 |L| / h both stay below 1e-9 |f'''| resp. 1e-10 |L|; the bar is 1e-6 of the largest
    gradient entry of the rows compared."""
    F, hw = 257, (16, 32)
    p = problem(F, hw)
    r = PR.shade_ref(p, mode, F64)
    rows = PR.mask_of(p["lab"]["cos"], "front") & PR.mask_of(p["lab"]["rough"], "mid")
    assert int(rows.sum()) >= 32

    def row_loss(q):
        o = PR.shade_ref(q, mode, F64, used=(False,) * 3)
        return sum((p["ups"][k].double() * o[name]).sum(-1) for k, name in enumerate(("Lo", "Lo_diff", "Lo_spec")))

    h = 1e-6
    for key, gname, cols in (("n", "g_normal", 3), ("albedo", "g_albedo", 3), ("rough", "g_roughness", 1), ("metal", "g_metallic", 1)):
        for c in range(cols):
            lp, lm = [], []
            for sgn, acc in ((1.0, lp), (-1.0, lm)):
                q = dict(p)
                x = p[key].double().clone()
                if cols == 3:
                    x[:, c] += sgn * h
                else:
                    x += sgn * h
                q[key] = x
                acc.append(row_loss(q))
            fd = (lp[0] - lm[0]) / (2 * h)
            g = r[gname][:, c] if cols == 3 else r[gname]
            assert float((fd - g)[rows].abs().max()) <= 1e-6 * float(r[gname][rows].abs().max()), (key, c)
    g_env = r["g_env"]
    flat = g_env.abs().flatten().argsort(descending=True)[:4].tolist() + [0, 16 * 32 * 3 - 1]
    for e in flat:
        ls = []
        for sgn in (1.0, -1.0):
            q = dict(p)
            b = p["base"].double().clone()
            b.view(-1)[e] += sgn * 1e-4                     # L is linear in a texel: any step is exact up to rounding
            q["base"] = b
            ls.append(row_loss(q).sum())
        fd = (ls[0] - ls[1]) / 2e-4
        assert abs(float(fd - g_env.view(-1)[e])) <= 1e-6 * float(g_env.abs().max()), e


@pytest.mark.parametrize("lobes", [1, 2, 3])
def test_scatterer_reference_selects_the_lobes(lobes):
    p = problem(257, (1, 1))
    g = PR.seeded(5)
    ups = [torch.randn(257, 1, generator=g), torch.randn(257, 3, generator=g)]
    r64, t32 = PR.scatterer_ref(p, lobes, F64, ups), PR.scatterer_ref(p, lobes, F32, ups)
    unlit = ~(PR.mask_of(p["lab"]["cos"], "front", "nov_neg"))
    for r in (r64, t32):
        assert bool((r["diff"][unlit] == 0).all()) and bool((r["spec"][unlit] == 0).all())
        assert bool((r["g_normal"][unlit] == 0).all())
        assert float(r["g_normal"].abs().max()) > 0
        if lobes == 1:
            assert float(r["spec"].abs().max()) == 0
            for k in ("g_roughness", "g_albedo", "g_metallic"):
                assert float(r[k].abs().max()) == 0
        else:
            assert float(r["spec"].abs().max()) > 0 and (lobes == 3) == (float(r["diff"].abs().max()) > 0)
            for k in ("g_roughness", "g_albedo", "g_metallic"):
                assert float(r[k].abs().max()) > 0
