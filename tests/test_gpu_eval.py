"""GPU (MI355X): the two model switches of the reference's test step on RenderStep -- `albedo_only` (models/intrinsic_avatar.py:222, :1290)
and `albedo_align_ratio` (:1114-1115) -- against the reference's own forward_ runs with them (tests/golden/golden_eval.npz, made by
tests/golden/make_golden_eval.py on the scene of golden_forward.npz), and system.evaluate_frame (systems/intrinsic_avatar.py:317-421,
:597-720) against the same pieces called by hand in the reference's order.

Bars against the reference's runs: those the suite already holds for the same run and key (tests/test_gpu_forward_golden.py: BARS_EVAL,
BARS_MC[run], the discrete-output rules of _check_common); the ratio's components are <= 1, so an albedo difference cannot grow.
The ratio runs draw their own light directions and shuffles, so a Monte-Carlo key (comp_rgb_phys*, comp_demod_phys*) whose maximum is set
by another flipped visibility sample may not fit the bar of the plain run: such a key -- and only such a key -- takes its bar from
tests/golden/eval_parity_bars.json (`visibility` of uniform_light included), 3 x the (max, p99, mean) observed on the MI355X, under the hard cap MC_CAP:
the largest bar the suite holds for that key over all evaluation runs.  The file is made by

    IA_EVAL_PARITY_OBSERVE=eval_parity_obs.json python -m pytest -m gpu tests/test_gpu_eval.py -k ratio      (on the MI355X)
    python -m tests.test_gpu_eval eval_parity_obs.json"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import forward_golden as FG
from tests.test_gpu_forward_golden import BARS_EVAL, BARS_MC, _check_common, _held

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BASES = ("light_16_nogi", "uniform_light_512_gi")
# keys of the output dict that the secondary branch decides
SECONDARY = ("comp_rgb_phys", "comp_demod_phys", "visibility")


EVAL_BARS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_parity_bars.json")
EVAL_BARS = json.load(open(EVAL_BARS_PATH))["bars"] if os.path.exists(EVAL_BARS_PATH) else {}
_OBSERVE = os.environ.get("IA_EVAL_PARITY_OBSERVE")
MC_KEYS = ("comp_rgb_phys", "comp_demod_phys", "comp_rgb_phys_full", "comp_demod_phys_full")
MC_CAP = {k: tuple(max(BARS_MC[r][k][i] for r in FG.RUNS) for i in range(3)) for k in MC_KEYS}
VISIBILITY_BAR = (4.6e-3, 1.3e-5, 9.7e-6)                      # tests/test_gpu_forward_golden.py, uniform_light_512_gi
MC_CAP["visibility"] = tuple(json.load(open(os.path.join(os.path.dirname(EVAL_BARS_PATH), "parity_bars.json")))["bars"]["relight/uniform_light/visibility"])


def _plain_bar(base, k):
    return VISIBILITY_BAR if k == "visibility" else BARS_MC[base][k]


def _triple(a, b):
    err = np.abs(a.astype(np.float64) - b.astype(np.float64))
    err = err.reshape(err.shape[0], -1).max(-1)
    return (float(err.max()), float(np.quantile(err, 0.99)), float(err.mean()))


def _held_mc(tag, base, k, a, b):
    """a Monte-Carlo key of a ratio run: the plain run's bar, or (only where the file names the key) 3 x the observation under MC_CAP."""
    got = _triple(a, b)
    print(tag, k, "observed (max, p99, mean)", got)
    if _OBSERVE:
        old = json.load(open(_OBSERVE)) if os.path.exists(_OBSERVE) else {}
        old[f"{tag}/{k}"] = list(got)
        os.makedirs(os.path.dirname(os.path.abspath(_OBSERVE)), exist_ok=True)
        json.dump(old, open(_OBSERVE, "w"), indent=0, sort_keys=True)
        return
    bar = _plain_bar(base, k)
    own = EVAL_BARS.get(f"{tag}/{k}")
    if own is not None:
        bar = tuple(max(x, min(y, c)) for x, y, c in zip(bar, own, MC_CAP[k]))
    assert got[0] <= bar[0] and got[1] <= bar[1] and got[2] <= bar[2], (tag, k, got, bar)


def _check_ratio_run(d, ref, base, tag):
    """_check_common of tests/test_gpu_forward_golden.py with the Monte-Carlo keys through _held_mc."""
    for k in ref:
        assert tuple(d[k].shape) == ref[k].shape and N(d[k]).dtype == ref[k].dtype, k
    for k in ("comp_rgb_bg", "comp_albedo_bg", "comp_metallic_bg", "comp_roughness_bg"):
        np.testing.assert_allclose(N(d[k]).astype(np.float64), ref[k].astype(np.float64), atol=1e-7, err_msg=k)
    for k, bar in BARS_EVAL.items():
        _held(k, N(d[k]), ref[k], bar)
    for k in MC_KEYS:
        _held_mc(tag, base, k, N(d[k]), ref[k])
    hit = ref["rays_valid"][:, 0]
    for k in ("comp_rgb_phys", "comp_demod_phys"):
        a, b = N(d[k]), ref[k]
        assert abs(a[hit].mean() - b[hit].mean()) <= 2e-3 * abs(b[hit].mean()), (k, a[hit].mean(), b[hit].mean())


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().as_subclass(torch.Tensor).cpu().numpy()


class _Both:
    """golden_eval.npz first, golden_forward.npz behind it (the scene, the rays)."""

    def __init__(self, E, G):
        self.E, self.G = E, G

    def __getitem__(self, k):
        return self.E[k] if k in self.E.files else self.G[k]


@pytest.fixture(scope="module")
def GE():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from intrinsicavatar_amd import build
    build.build()
    E = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_eval.npz"))
    return FG.load(), E


def _draws(G, tag, mode):
    rnd = FG.explicit_randoms(G, tag)
    return T(rnd["stratified_u"] if mode == "uniform_light" else rnd["light_u"]), T(rnd["shuffle_u"])


def _ref(E, tag):
    return {str(k): E[f"{tag}_out_{k}"] for k in E[tag + "_out_keys"]}


@pytest.mark.parametrize("base", BASES)
def test_albedo_only_skips_the_secondary_branch_and_changes_nothing_else(GE, base):
    G, E = GE
    mode, spp, gi = FG.RUNS[base]
    rs, mat, env, rays = FG.gpu_scene(G, base)
    light_u, shuffle_u = _draws(G, base, mode)
    kw = dict(background_color=T(G["background_color"]), global_illumination=gi, render_mode=mode)
    full = rs.forward_(rays, mat, env, spp, light_u, shuffle_u, **kw)
    ao = rs.forward_(rays, mat, env, spp, light_u, shuffle_u, albedo_only=True, **kw)
    assert sorted(ao) == sorted(full)
    independent = [k for k in full if not k.startswith(SECONDARY)]
    for want in ("comp_rgb", "comp_rgb_bg", "comp_rgb_full", "comp_normal", "opacity", "depth", "comp_albedo", "comp_albedo_full", "comp_metallic",
                 "comp_metallic_full", "comp_roughness", "comp_roughness_full", "rays_valid", "rays_valid_phys", "rays_valid_full", "num_samples"):
        assert want in independent, want
    for k in independent:
        assert torch.equal(ao[k], full[k]), k                               # bit-identical to the full pass on the same rays and draws
    bg = T(G["background_color"])
    assert torch.equal(ao["comp_rgb_phys"], bg[None].expand(rays.shape[0], 3)) and torch.equal(ao["comp_demod_phys"], ao["comp_rgb_phys"])
    assert float((full["comp_rgb_phys"] - ao["comp_rgb_phys"]).abs().max()) > 1e-2            # the full pass did shade
    if mode == "uniform_light":
        assert float(ao["visibility"].abs().max()) == 0.0 and tuple(ao["visibility"].shape) == (rays.shape[0], 1)
    st = rs.relight(rays, mat, env, spp, light_u, shuffle_u, albedo_only=True, **kw)["stats"]
    assert st["n_secondary"] == 0 and st["n_resampled"] == 0 and st["n_fg"] == 0
    # against the reference's own run with model.albedo_only = True: key set, dtypes, values
    ref = _ref(E, base + "_albedo_only")
    assert sorted(ao) == sorted(ref), sorted(set(ao) ^ set(ref))
    for k in ref:
        assert N(ao[k]).dtype == ref[k].dtype, (k, N(ao[k]).dtype, ref[k].dtype)
    _check_common(ao, ref, base)
    for k in ("comp_rgb_phys", "comp_demod_phys"):
        assert np.array_equal(N(ao[k]), ref[k]), k
    assert int(ao["num_samples"][0]) == int(ref["num_samples"][0])
    for k in ("rays_valid", "rays_valid_phys", "rays_valid_full", "rays_valid_phys_full"):
        assert np.array_equal(N(ao[k]), ref[k]), k


@pytest.mark.parametrize("base", BASES)
def test_albedo_align_ratio_against_the_references_run(GE, base):
    G, E = GE
    mode, spp, gi = FG.RUNS[base]
    tag = base + "_ratio"
    rs, mat, env, rays = FG.gpu_scene(G, base)
    light_u, shuffle_u = _draws(_Both(E, G), tag, mode)
    kw = dict(background_color=T(G["background_color"]), global_illumination=gi, render_mode=mode)
    ratio = T(E["ratio"])
    assert float(ratio.max()) <= 1.0
    d = rs.forward_(rays, mat, env, spp, light_u, shuffle_u, albedo_align_ratio=ratio, **kw)
    ref = _ref(E, tag)
    assert sorted(d) == sorted(ref), sorted(set(d) ^ set(ref))
    _check_ratio_run(d, ref, base, tag)
    if mode == "uniform_light":
        _held_mc(tag, base, "visibility", N(d["visibility"]), ref["visibility"])
    # discrete outputs: identical
    assert int(d["num_samples"][0]) == int(ref["num_samples"][0])
    for k in ref:
        if ref[k].dtype.kind in "biu":
            assert np.array_equal(N(d[k]), ref[k]), k
    # the ratio scales the composited albedo and changes the shaded maps
    plain = rs.forward_(rays, mat, env, spp, light_u, shuffle_u, **kw)
    hit = N(plain["rays_valid"])[:, 0]
    np.testing.assert_allclose(N(d["comp_albedo"])[hit], N(plain["comp_albedo"])[hit] * E["ratio"][None], rtol=2e-5, atol=1e-7)
    assert float((d["comp_rgb_phys"] - plain["comp_rgb_phys"]).abs().max()) > 1e-3
    for k in ("comp_rgb", "comp_normal", "opacity", "depth", "comp_roughness", "comp_metallic"):
        assert torch.equal(d[k], plain[k]), k
    # ratio (1, 1, 1) is bit-identical to no ratio
    ones = rs.forward_(rays, mat, env, spp, light_u, shuffle_u, albedo_align_ratio=torch.ones(3, device=DEV), **kw)
    for k in plain:
        assert torch.equal(ones[k], plain[k]), k


def _frame(G, rs, mat, env, rays, light_u, shuffle_u, kw, with_hdri):
    """a 28 x 28 test batch after preprocess_data: targets derived from a first pass so that the masks are body-shaped."""
    from intrinsicavatar_amd import metrics as M
    first = rs.forward_(rays, mat, env, 16, light_u, shuffle_u, **kw)
    n = rays.shape[0]
    g = torch.Generator().manual_seed(5)
    noise = lambda *s: torch.rand(s, generator=g).to(DEV)      # noqa: E731
    w2c = torch.eye(4, device=DEV)
    w2c[:3, :3] = torch.linalg.qr(torch.randn((3, 3), generator=g))[0].to(DEV)
    alpha = (first["opacity"][:, 0] > 0.5).float() * 0.9 + 0.05
    # target normals: the camera-space prediction turned by atan(0.5) = 26.6 degrees on every pixel (acos stays well conditioned)
    cam0 = M.transform_normals(first["comp_normal"], w2c[None])
    perp = torch.cross(cam0, torch.nn.functional.one_hot(cam0.abs().argmin(-1), 3).float(), dim=-1)
    perp = perp / perp.norm(dim=-1, keepdim=True).clamp_min(1e-20) * cam0.norm(dim=-1, keepdim=True)
    batch = dict(rays=rays, rgb=(first["comp_rgb_phys_full"] + 0.05 * (noise(n, 3) - 0.5)).clamp(0, 1), alpha=alpha,
                 valid_mask=first["opacity"][:, 0] > 0.1, albedo=(first["comp_albedo_full"] * 1.3 + 0.02 * noise(n, 3)).clamp(0, 1),
                 normal=cam0 + 0.5 * perp, w2c=w2c[None])
    if with_hdri:
        batch["hdri"] = T(G["hdri"])
    return batch


def test_evaluate_frame_is_the_pieces_in_the_references_order(GE):
    from intrinsicavatar_amd import metrics as M, system
    G, E = GE
    base = "light_16_nogi"
    rs, mat, env, rays = FG.gpu_scene(G, base)
    light_u, shuffle_u = _draws(G, base, "light")
    kw = dict(background_color=T(G["background_color"]), global_illumination=False, render_mode="light")
    H = W = 28
    batch = _frame(G, rs, mat, env, rays, light_u, shuffle_u, kw, with_hdri=True)
    gm, vm = batch["alpha"] > 0.5, batch["valid_mask"]
    assert int(gm.sum()) > 49 and int(vm.sum()) >= int(gm.sum())
    # ---- by hand, in the reference's order: albedo-only pass -> ratio -> full pass -> metrics
    pred = rs.forward_(rays, mat, env, 16, light_u, shuffle_u, albedo_only=True, **kw)["comp_albedo_full"]
    ratio = M.compute_albedo_rescale_factor(batch["albedo"], pred, gm)
    out = rs.forward_(rays, mat, env, 16, light_u, shuffle_u, albedo_align_ratio=ratio, **kw)
    img = lambda t: t.reshape(H, W, 3)      # noqa: E731
    psnr, ssim, nerr = M.PSNR(), M.SSIM(), M.NormalError()
    cam = M.transform_normals(out["comp_normal"], batch["w2c"])
    F = torch.nn.functional
    hand = dict(rf_psnr=psnr(out["comp_rgb_full"], batch["rgb"], valid_mask=vm),
                rf_ssim=ssim(img(out["comp_rgb_full"]), img(batch["rgb"]), valid_mask=vm.reshape(H, W)),
                pbr_psnr=psnr(out["comp_rgb_phys_full"], batch["rgb"], valid_mask=vm),
                pbr_ssim=ssim(img(out["comp_rgb_phys_full"]), img(batch["rgb"]), valid_mask=vm.reshape(H, W)),
                albedo_psnr=psnr(out["comp_albedo_full"], batch["albedo"], valid_mask=gm),
                albedo_ssim=ssim(img(out["comp_albedo_full"]), img(batch["albedo"]), valid_mask=gm.reshape(H, W)))
    hand_normal = nerr(F.normalize(cam, dim=-1), F.normalize(batch["normal"], dim=-1), gm)
    # ---- evaluate_frame; host synchronisations are only allowed inside the model's forward passes
    calls = []
    inner = system.model_forward

    def counted(*a, **k):
        torch.cuda.set_sync_debug_mode("default")
        try:
            calls.append(1)
            return inner(*a, **k)
        finally:
            torch.cuda.set_sync_debug_mode("error")
    system.model_forward = counted
    torch.cuda.set_sync_debug_mode("error")
    try:
        metrics, res = system.evaluate_frame(rs, dict(batch), mat, env, 16, light_u, shuffle_u, img_wh=(W, H), stage="test", **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        system.model_forward = inner
    assert len(calls) == 2                                              # the albedo-only pass and the full pass
    assert sorted(metrics) == sorted(system.METRIC_KEYS) and not any(k.endswith("lpips") for k in metrics)
    for k, v in hand.items():
        assert v.is_cuda and metrics[k].is_cuda and metrics[k].dim() == 0
        assert N(metrics[k]).tobytes() == N(v).tobytes(), (k, float(metrics[k]), float(v))
    assert N(metrics["rf_ssim"]).dtype == np.float64 and N(metrics["rf_psnr"]).dtype == np.float32
    # the fused transform + normalise + error kernel agrees with the three separate calls (same float32 operations per pixel)
    assert abs(float(metrics["normal_error"]) - float(hand_normal)) <= 2e-3
    assert torch.equal(res["comp_normal"], cam) and torch.equal(res["aligned_albedo"], out["comp_albedo_full"])
    for k in ("comp_rgb_full", "comp_rgb_phys_full", "comp_albedo_full"):
        assert res[k].is_cuda and torch.equal(res[k], out[k]), k
    host = M.to_host(metrics)                                           # one read-back for all of them
    assert sorted(host) == sorted(metrics) and all(np.isfinite(v) for v in host.values())
    assert host["rf_psnr"] == float(metrics["rf_psnr"]) and host["albedo_ssim"] == float(metrics["albedo_ssim"])
    print("evaluate_frame", host)
    # ---- without an HDRI: one full pass, alignment afterwards
    batch2 = _frame(G, rs, mat, env, rays, light_u, shuffle_u, kw, with_hdri=False)
    metrics2, res2 = system.evaluate_frame(rs, dict(batch2), mat, env, 16, light_u, shuffle_u, img_wh=(W, H), stage="test", **kw)
    assert sorted(metrics2) == sorted(system.METRIC_KEYS)
    plain = rs.forward_(rays, mat, env, 16, light_u, shuffle_u, **kw)
    assert torch.equal(res2["comp_albedo_full"], plain["comp_albedo_full"])           # no ratio inside the model
    al = res2["aligned_albedo"]
    want, r2 = M.align_albedo(batch2["albedo"], plain["comp_albedo_full"], gm)
    assert torch.equal(al, want) and float(al.min()) >= 0.0 and float(al.max()) <= 1.0 and float(al[~gm].abs().max()) == 0.0
    assert not torch.equal(al, plain["comp_albedo_full"])
    assert N(metrics2["albedo_psnr"]).tobytes() == N(psnr(want, batch2["albedo"], valid_mask=gm)).tobytes()
    # validation stage never runs the albedo-only pass, HDRI or not
    metrics3, _ = system.evaluate_frame(rs, dict(batch), mat, env, 16, light_u, shuffle_u, img_wh=(W, H), stage="validation", **kw)
    assert N(metrics3["albedo_psnr"]).tobytes() == N(metrics2["albedo_psnr"]).tobytes()


def _make_bars(obs_path):
    """tests/golden/eval_parity_bars.json from an observation run: only the keys that do not fit the plain run's bar, at 3 x observed."""
    obs = json.load(open(obs_path))
    bars = {}
    for name, got in sorted(obs.items()):
        tag, k = name.split("/")
        base = tag[:-len("_ratio")]
        if any(g > b for g, b in zip(got, _plain_bar(base, k))):
            bars[name] = [3.0 * g for g in got]
    json.dump(dict(note="3 x the MI355X observation, (max, p99, mean) of the per-pixel absolute difference to the reference's run; only the "
                        "Monte-Carlo keys of the albedo_align_ratio runs that do not fit the bar of the plain run (tests/test_gpu_eval.py)",
                   command=["IA_EVAL_PARITY_OBSERVE=eval_parity_obs.json python -m pytest -m gpu tests/test_gpu_eval.py -k ratio",
                            "python -m tests.test_gpu_eval eval_parity_obs.json"],
                   observed={k: obs[k] for k in bars}, bars=bars), open(EVAL_BARS_PATH, "w"), indent=0, sort_keys=True)
    print(len(bars), "bars ->", EVAL_BARS_PATH)


if __name__ == "__main__":
    _make_bars(sys.argv[1])
