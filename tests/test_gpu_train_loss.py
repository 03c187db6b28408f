"""GPU: the fused training loss (ia_train_loss / ia_train_loss_bwd, intrinsicavatar_amd/train_loss.py) against
train_phys.reference_training_loss + mean |laplace|, evaluated in fp64 with autograd on CPU copies of the same fp32 inputs.

Bounds (derived, not measured): every summand is formed from fp32 inputs with fewer than ten roundings of 6e-8 and summed in fp64, and
no term of these inputs cancels (gradient norms stay 0.02 away from 1, targets differ from predictions), so every term and the loss
agree to 1e-5 relative and every gradient tensor to 1e-5 of its largest reference entry.

MAX_BLOCKS: csrc/train_loss.hip reduces with at most 1024 blocks of 256 rows over the samples (and as many over the rays); above
1024 * 256 = 262 144 samples a block's threads stride over more than one row each -- N_ABOVE_CAP is past that."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_BLOCKS, TB = 1024, 256
N_ABOVE_CAP = MAX_BLOCKS * TB + 4097
RAYS = (1, 63, 64, 65, 257)
SAMPLES = (1, 255, 256, 257, 70_001, N_ABOVE_CAP)
REL = 1e-5
MAPS = ("normals_orientation_loss_map", "albedo_smoothness_loss_map", "roughness_smoothness_loss_map", "metallic_smoothness_loss_map")
DIFF = ("comp_rgb_full", "comp_rgb_phys_full", "comp_demod_phys_full", "opacity") + MAPS + ("sdf_samples", "sdf_grad_samples",
                                                                                           "sdf_laplace_samples")
ALL_ON = dict(lambda_rgb_mse=0.7, lambda_rgb_l1=1.0, lambda_rgb_phys_mse=0.3, lambda_rgb_phys_l1=0.2, lambda_rgb_demodulated=0.4,
              lambda_eikonal=0.1, lambda_mask_mse=0.6, lambda_mask_bce=0.1, lambda_opaque=0.05, lambda_sparsity=0.9, lambda_curvature=1.5,
              lambda_normal_orientation=0.8, lambda_albedo_smoothness=0.01, lambda_roughness_smoothness=0.02,
              lambda_metallic_smoothness=0.03, sparsity_scale=1.7)


class _Material:
    """what reference_training_loss asks of the material: VolumeMaterial.regularizations' map means (the real method; the Lipschitz
    bound, a function of parameters this test has none of, is a constant here and never weighted)"""

    def lipshitz_bound_full(self):
        return torch.zeros(1, dtype=torch.float64)

    def regularizations(self, out=None):
        from intrinsicavatar_amd import fields
        return fields.VolumeMaterial.regularizations(self, out)


def make_inputs(n, m, seed=0, valid_none=False):
    """fp32 CPU tensors: (out dict, rgb, alpha, rgb_wo_mask)"""
    g = torch.Generator().manual_seed(seed * 1000003 + n * 131 + m)
    r = lambda *s: torch.rand(*s, generator=g)      # noqa: E731
    out = {}
    for k in ("comp_rgb_full", "comp_rgb_phys_full", "comp_demod_phys_full"):
        out[k] = r(n, 3)
    op = r(n, 1)
    special = torch.tensor([0.0, 1.0e-3, 1.0 - 1.0e-3, 1.0, 0.5e-3, 1.0 - 0.5e-3])[:n]
    op[:special.shape[0], 0] = special
    out["opacity"] = op
    for k in MAPS:
        out[k] = r(n, 1) * 2.0
    v, vp = r(n, 1) < 0.7, r(n, 1) < 0.6
    if valid_none:
        v[:], vp[:] = False, False
    else:
        v[n // 2], vp[(n // 2 + 1) % n] = True, True
    out["rays_valid_full"], out["rays_valid_phys_full"] = v, vp
    sdf = (r(m) - 0.5) * 0.4
    sdf[::7] = 1.0e5                                             # samples without a valid root
    out["sdf_samples"] = sdf
    d = torch.nn.functional.normalize(torch.randn(m, 3, generator=g), dim=-1)
    u = r(m)
    norm = torch.where(u < 0.5, 0.5 + 0.96 * u, 1.02 + 0.96 * (u - 0.5))      # [0.5, 0.98) and [1.02, 1.5)
    out["sdf_grad_samples"] = d * norm[:, None]
    out["sdf_laplace_samples"] = (r(m) - 0.3) * 0.2
    rgb, rgb_wo_mask = r(n, 3), r(n, 3)
    alpha = (r(n) < 0.5).float()
    alpha[::5] = r(n)[::5]                                       # soft mask values as well
    return out, rgb, alpha, rgb_wo_mask


def reference(out, rgb, alpha, lam, rgb_wo_mask=None, drop=()):
    """fp64 CPU: (loss, terms, {input: gradient or None})"""
    from intrinsicavatar_amd import train_phys
    o = {k: (v.double().requires_grad_(True) if v.dtype == torch.float32 else v) for k, v in out.items() if k not in drop}
    d = lambda t: t.double() if t is not None else None      # noqa: E731
    loss, t = train_phys.reference_training_loss(o, d(rgb), d(alpha), lam, _Material(), d(rgb_wo_mask))
    if "sdf_laplace_samples" in o:
        t["curvature"] = o["sdf_laplace_samples"].abs().mean()
        if lam.get("lambda_curvature", 0.0):
            loss = loss + lam["lambda_curvature"] * t["curvature"]
    t.pop("lipshitz_bound", None)
    names = [k for k in DIFF if k in o]
    grads = torch.autograd.grad(loss, [o[k] for k in names], allow_unused=True) if torch.is_tensor(loss) and loss.requires_grad else [None] * len(names)
    return loss, t, dict(zip(names, grads))


def fused(out, rgb, alpha, lam, rgb_wo_mask=None, drop=()):
    from intrinsicavatar_amd import train_loss
    dev = torch.device("cuda")
    o = {k: (v.to(dev).requires_grad_(True) if v.dtype == torch.float32 else v.to(dev)) for k, v in out.items() if k not in drop}
    c = lambda t: t.to(dev) if t is not None else None      # noqa: E731
    loss, t = train_loss.fused_reference_loss(o, c(rgb), c(alpha), lam, None, c(rgb_wo_mask))
    if loss.requires_grad:
        loss.backward()
    return loss.detach(), t, {k: o[k].grad for k in DIFF if k in o}


def compare(ref, got, what):
    (l0, t0, g0), (l1, t1, g1) = ref, got
    assert set(t0) == set(t1), (what, sorted(t0), sorted(t1))
    val = lambda v: float(v.detach()) if torch.is_tensor(v) else float(v)      # noqa: E731
    rows = [("loss", val(l0), val(l1))] + [(k, val(t0[k]), val(t1[k])) for k in t0]
    for k, a, b in rows:
        print(f"{what} {k}: reference {a!r} fused {b!r}")
        assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= REL * abs(a), (what, k, a, b)
    for k, ga in g0.items():
        gb = g1[k]
        if ga is None or float(ga.abs().max()) == 0.0:
            assert gb is None or float(gb.abs().max()) == 0.0, (what, k)
            continue
        assert gb is not None, (what, k)
        err, top = float((gb.cpu().double() - ga).abs().max()), float(ga.abs().max())
        print(f"{what} d/d{k}: max error {err:.3e}, largest reference entry {top:.3e}")
        assert gb.shape == ga.shape and err <= REL * top, (what, k, err, top)


@pytest.mark.parametrize("n", RAYS)
@pytest.mark.parametrize("m", SAMPLES)
def test_all_terms_at_every_shape(n, m):
    inp = make_inputs(n, m)
    compare(reference(*inp[:3], ALL_ON), fused(*inp[:3], ALL_ON), f"n={n} m={m}")


@pytest.mark.parametrize("term", [k[len("lambda_"):] for k in ALL_ON if k.startswith("lambda_")])
def test_every_term_alone(term):
    inp = make_inputs(65, 257, seed=1)
    lam = {"lambda_" + term: 1.0, "sparsity_scale": 1.7}
    ref, got = reference(*inp[:3], lam), fused(*inp[:3], lam)
    compare(ref, got, term)
    assert abs(float(got[0]) - float(got[1][term])) <= 1e-6 * abs(float(got[1][term]))


def test_rgb_wo_mask_form():
    """add_emitter: the PBR terms run over ALL rays against the unmasked image"""
    out, rgb, alpha, wo = make_inputs(65, 257, seed=2)
    compare(reference(out, rgb, alpha, ALL_ON, wo), fused(out, rgb, alpha, ALL_ON, wo), "rgb_wo_mask")
    plain = fused(out, rgb, alpha, ALL_ON)
    assert float(plain[1]["rgb_phys_l1"]) != float(fused(out, rgb, alpha, ALL_ON, wo)[1]["rgb_phys_l1"])


def test_absent_inputs_are_null_pointers():
    """no alpha (no mask terms, no opaque), no smoothness maps, no laplace: the terms are absent on both routes"""
    out, rgb, _, _ = make_inputs(65, 257, seed=3)
    drop = MAPS + ("sdf_laplace_samples",)
    ref, got = reference(out, rgb, None, ALL_ON, drop=drop), fused(out, rgb, None, ALL_ON, drop=drop)
    compare(ref, got, "absent")
    assert not {"mask_bce", "opaque", "curvature", "albedo_smoothness"} & set(got[1])
    assert got[2]["opacity"] is None


def test_no_valid_ray_gives_nan_where_torch_does():
    out, rgb, alpha, _ = make_inputs(65, 257, seed=4, valid_none=True)
    ref, got = reference(out, rgb, alpha, ALL_ON), fused(out, rgb, alpha, ALL_ON)
    nan = {k for k, v in ref[1].items() if math.isnan(float(v))}
    assert nan == {"rgb_mse", "rgb_l1", "rgb_phys_mse", "rgb_phys_l1", "rgb_demodulated"}
    assert nan == {k for k, v in got[1].items() if math.isnan(float(v))}
    assert math.isnan(float(ref[0])) and math.isnan(float(got[0]))
    lam = {k: v for k, v in ALL_ON.items() if k[len("lambda_"):] not in nan}      # NaN terms without a weight stay out of the loss
    compare(reference(out, rgb, alpha, lam), fused(out, rgb, alpha, lam), "no valid ray, NaN terms unweighted")


def test_zero_weight_gives_no_gradient():
    inp = make_inputs(65, 257, seed=5)
    lam = dict(lambda_rgb_l1=1.0, lambda_eikonal=0.1, lambda_curvature=0.0, lambda_mask_bce=0.0, sparsity_scale=1.0)
    _, terms, grads = fused(*inp[:3], lam)
    assert grads["comp_rgb_full"] is not None and grads["sdf_grad_samples"] is not None
    for k in DIFF:
        if k not in ("comp_rgb_full", "sdf_grad_samples"):
            assert grads[k] is None, k
    assert float(terms["curvature"]) > 0.0          # the value is still reported


def test_two_calls_give_the_same_bits():
    inp = make_inputs(257, 70_001, seed=6)
    a, b = fused(*inp[:3], ALL_ON), fused(*inp[:3], ALL_ON)
    assert a[0].view(torch.int32).item() == b[0].view(torch.int32).item()
    for k in a[1]:
        assert torch.equal(a[1][k].view(torch.int32), b[1][k].view(torch.int32)), k
    for k in DIFF:
        assert torch.equal(a[2][k].view(torch.int32), b[2][k].view(torch.int32)), k


def test_partials_query():
    from intrinsicavatar_amd import _lib as L
    q = lambda n, m: int(L.lib().ia_train_loss_partials(L.i64(n), L.i64(m)))      # noqa: E731
    assert q(0, 0) == 0 and q(-1, 0) == -1
    assert q(1, 1) == 14 + 3 and q(257, 0) == 2 * 14
    assert q(0, N_ABOVE_CAP) == MAX_BLOCKS * 3 == q(0, MAX_BLOCKS * TB)
