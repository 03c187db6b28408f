"""CPU: the parts of model.add_emitter that need no GPU -- the new entry points in the header and the library, the defaults of every new
argument (today's behaviour), reference_training_loss(rgb_wo_mask=...), and the consistency of tests/golden/golden_emitter.npz (the
reference's forward_ with add_emitter, tests/golden/make_golden_emitter.py) with golden_forward.npz.  Kernels and end to end:
tests/test_gpu_emitter_background.py."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("ia_envlight_background", "ia_envlight_background_bwd", "ia_transform_dirs_s2w",
       "ia_vi_composite_bwd_bg")


def test_entry_points_are_declared_and_exported():
    from intrinsicavatar_amd import _lib, build
    protos = _lib.header_prototypes()
    so = C.CDLL(build.build())
    for name in NEW:
        assert name in protos, name
        assert hasattr(so, name), name
    assert len(protos["ia_envlight_background"][1]) == 8 and len(protos["ia_envlight_background_bwd"][1]) == 10
    assert len(protos["ia_vi_composite_bwd_bg"][1]) == 7
    # the signature existing tests call stays
    assert len(protos["ia_vi_composite_bwd"][1]) == 14 and len(protos["ia_vi_composite"][1]) == 12


def test_backward_takes_no_sized_work_area():
    """its two integer buffers have the shapes of its arguments ([H,W,3] int64, [1] uint32): no size query to get wrong"""
    from intrinsicavatar_amd import _lib
    protos = _lib.header_prototypes()
    assert not [n for n in protos if n.startswith("ia_envlight_background") and n.endswith("_bytes")]
    args = protos["ia_envlight_background_bwd"][1]
    assert args[-1] is C.c_void_p and C.c_size_t not in args


def test_new_arguments_default_to_todays_behaviour():
    from intrinsicavatar_amd import animation, pbr, render, train_phys
    sig = lambda f: inspect.signature(f).parameters      # noqa: E731
    for f in (render.RenderStep.relight, render.RenderStep.forward_, render.RenderStep.forward_train_, train_phys.shade_differentiable_phys,
              animation.render_sequence):
        assert sig(f)["add_emitter"].default is False, f
    assert sig(pbr.VolumeInteraction.composite)["background_rays"].default is None
    assert sig(train_phys.reference_training_loss)["rgb_wo_mask"].default is None
    assert sig(animation.render_sequence)["resample_light"].default is True
    for cls in (pbr.EnvironmentLightTensor, pbr.EnvironmentLightSG):
        assert list(sig(cls.background))[:3] == ["self", "rays_d_smpl", "w2s_rot"]


class _Material:
    def regularizations(self, out):
        return {}


def _training_dict(n, g):
    r = lambda *s: torch.rand(s, generator=g)      # noqa: E731
    valid = r(n, 1) > 0.4
    return dict(comp_rgb_full=r(n, 3), comp_rgb_phys_full=r(n, 3).requires_grad_(True), comp_demod_phys_full=r(n, 3), rays_valid_full=valid,
                rays_valid_phys_full=valid, sdf_grad_samples=r(50, 3), sdf_samples=r(50), opacity=r(n, 1))


def test_reference_training_loss_over_all_rays_against_the_unmasked_image():
    """systems/intrinsic_avatar.py:184-203: with add_emitter the two physically based terms are means over ALL rays against rgb_wo_mask;
    every other term stays as it is"""
    from intrinsicavatar_amd import train_phys
    g = torch.Generator().manual_seed(3)
    n = 40
    out = _training_dict(n, g)
    rgb, wo, alpha = torch.rand((n, 3), generator=g), torch.rand((n, 3), generator=g), (torch.rand(n, generator=g) > 0.5).float()
    lam = dict(lambda_rgb_phys_l1=1.0, lambda_rgb_phys_mse=2.0, lambda_rgb_l1=0.5, lambda_eikonal=0.1)
    l0, t0 = train_phys.reference_training_loss(out, rgb, alpha, lam, _Material())
    l1, t1 = train_phys.reference_training_loss(out, rgb, alpha, lam, _Material(), rgb_wo_mask=wo)
    vp = out["rays_valid_phys_full"][:, 0]
    F = torch.nn.functional
    full = out["comp_rgb_phys_full"]
    assert torch.equal(t0["rgb_phys_l1"], F.l1_loss(full[vp], rgb[vp])) and torch.equal(t0["rgb_phys_mse"], F.mse_loss(full[vp], rgb[vp]))
    assert torch.equal(t1["rgb_phys_l1"], F.l1_loss(full, wo)) and torch.equal(t1["rgb_phys_mse"], F.mse_loss(full, wo))
    assert set(t0) == set(t1)
    for k in t0:
        if k not in ("rgb_phys_l1", "rgb_phys_mse"):
            assert torch.equal(t0[k], t1[k]), k
    # rays outside the valid mask receive gradient only in the all-rays form
    g0, = torch.autograd.grad(l0, full, retain_graph=True)
    g1, = torch.autograd.grad(l1, full)
    assert float(g0[~vp].abs().max()) == 0.0 and float(g1[~vp].abs().min()) > 0.0


RUNS = {"light_16_nogi": "light_16_nogi", "uniform_light_512_gi": "uniform_light_512_gi", "mis_16_gi": "mis_16_gi",
        "light_16_nogi_albedo_only": "light_16_nogi"}


@pytest.mark.parametrize("tag", list(RUNS))
def test_golden_emitter_fixture(tag):
    """data only: four maps per run, shaped like the ones of golden_forward.npz; rays the reference left without any opacity carry the
    emitter's radiance (the fp64 bilinear expression within fp32 rounding of a map that reaches 40), and at least a third of the rays moved"""
    GE = np.load(os.path.join(HERE, "golden", "golden_emitter.npz"))
    GF = np.load(os.path.join(HERE, "golden", "golden_forward.npz"))
    assert sorted(GE.files) == sorted(f"{t}_{k}" for t in RUNS for k in ("comp_rgb_phys", "comp_demod_phys", "comp_rgb_phys_full", "comp_demod_phys_full"))
    src = RUNS[tag]
    for k in ("comp_rgb_phys", "comp_demod_phys", "comp_rgb_phys_full", "comp_demod_phys_full"):
        a, b = GE[f"{tag}_{k}"], GF[f"{src}_out_{k}"]
        assert a.shape == b.shape == (784, 3) and a.dtype == b.dtype == np.float32 and np.isfinite(a).all()
    moved = np.abs(GE[f"{tag}_comp_rgb_phys"] - GF[f"{src}_out_comp_rgb_phys"]).max(-1) > 0
    assert moved.sum() > 784 // 3
    empty = GF[f"{src}_out_opacity"][:, 0] == 0
    assert empty.sum() > 200
    # E along the camera rays: d_world = normalize(d_smpl @ w2s[:3,:3]), d_smpl = d @ w2s[:3,:3]^T  ->  the world direction itself
    d = GF["rays"][:, 3:6].astype(np.float64)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    base = GF["hdri"].astype(np.float64)
    H, W, _ = base.shape
    u = np.arctan2(d[:, 0], -d[:, 2]) / (2 * np.pi) + 0.5
    v = np.arccos(np.clip(d[:, 1], -1, 1)) / np.pi
    fx, fy = u * W - 0.5, v * H - 0.5
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    ax, ay = (fx - x0)[:, None], (fy - y0)[:, None]
    x1, y1 = (x0 + 1) % W, np.clip(y0 + 1, 0, H - 1)
    x0, y0 = x0 % W, np.clip(y0, 0, H - 1)
    E = (1 - ax) * (1 - ay) * base[y0, x0] + ax * (1 - ay) * base[y0, x1] + (1 - ax) * ay * base[y1, x0] + ax * ay * base[y1, x1]
    got = GE[f"{tag}_comp_rgb_phys"].astype(np.float64)
    # the rotation there and back, the normalisation and the fp32 lookup: 1e-5 of the map's range per unit of its steepest neighbour step
    step = max(np.abs(base - np.roll(base, -1, 1)).max(), np.abs(base[1:] - base[:-1]).max())
    assert np.abs(got[empty] - E[empty]).max() <= 1e-5 * step * max(H, W) + 1e-6 * base.max()
