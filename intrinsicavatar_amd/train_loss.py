"""The loss of IntrinsicAvatarSystem.training_step (systems/intrinsic_avatar.py:160-301) as ONE autograd node on ia_train_loss /
ia_train_loss_bwd: two launches forward and one backward instead of the ~100 element-wise / index / reduce launches of
train_phys.reference_training_loss and its autograd graph.  Same terms, same conventions (the RGB means over the valid rays, the
clamped opacity, NaN for a mean over nothing), plus `curvature` = mean |sdf_laplace_samples| (:265-268).

Every mean is summed in fp64 in a fixed order (csrc/train_loss.hip): a call's result does not depend on what ran before it.
`albedo_entropy` (a histogram, not a mean) stays in fields.VolumeMaterial.regularizations and is added here in Python; the Lipschitz
bound is a function of the material's parameters alone and is added by the caller (fit.Trainer)."""
import ctypes as C
from typing import Dict, Optional

import torch
from torch import Tensor
from torch.autograd import Function

from . import _lib as L
from . import fields

# order of terms[] / weights[] in include/ia_amd.h (slot 15 is unused)
TERMS = ("rgb_mse", "rgb_l1", "rgb_phys_mse", "rgb_phys_l1", "rgb_demodulated", "eikonal", "mask_mse", "mask_bce", "opaque", "sparsity",
         "curvature", "normal_orientation", "albedo_smoothness", "roughness_smoothness", "metallic_smoothness")
N_TERMS, N_STATS = 16, 18
_MAPS = ("normals_orientation_loss_map", "albedo_smoothness_loss_map", "roughness_smoothness_loss_map", "metallic_smoothness_loss_map")
# differentiable inputs of _TrainLoss, in argument order, with the terms that depend on each
_DIFF = (("comp_rgb_full", (0, 1)), ("comp_rgb_phys_full", (2, 3)), ("comp_demod_phys_full", (4,)), ("opacity", (6, 7, 8)),
         (_MAPS[0], (11,)), (_MAPS[1], (12,)), (_MAPS[2], (13,)), (_MAPS[3], (14,)), ("sdf_samples", (9,)), ("sdf_grad_samples", (5,)),
         ("sdf_laplace_samples", (10,)))
_N_CONST = 7          # weights, sparsity_scale, rgb, rgb_wo_mask, alpha, rays_valid_full, rays_valid_phys_full


def _f(t: Optional[Tensor]) -> Optional[Tensor]:
    return t.detach().float().contiguous() if t is not None else None


def _u8(t: Optional[Tensor]) -> Optional[Tensor]:
    if t is None:
        return None
    t = t.detach().reshape(-1).contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t.to(torch.uint8)


class _TrainLoss(Function):
    """(weights [16 floats], sparsity_scale, rgb, rgb_wo_mask, alpha, rays_valid_full, rays_valid_phys_full, then the eleven differentiable
    inputs of _DIFF; None = absent) -> (loss [], terms [16]).  A gradient comes back only for an input that some term of non-zero
    weight reads; every other one is None."""

    @staticmethod
    def forward(ctx, weights, sparsity_scale, rgb, rgb_wo_mask, alpha, valid, valid_phys, *diff):
        assert len(diff) == len(_DIFF) and len(weights) == N_TERMS
        shapes = [tuple(t.shape) if t is not None else None for t in diff]
        diff = [_f(t) for t in diff]
        rgb, rgb_wo_mask, alpha, valid, valid_phys = _f(rgb), _f(rgb_wo_mask), _f(alpha), _u8(valid), _u8(valid_phys)
        per_ray = [t for t in diff[:8] + [rgb, rgb_wo_mask] if t is not None]
        n = max([t.numel() // 3 if (t.dim() == 2 and t.shape[-1] == 3) else t.numel() for t in per_ray] or [0])
        sdf, sdf_grad, lap = diff[8], diff[9], diff[10]
        m = sdf_grad.numel() // 3 if sdf_grad is not None else max([t.numel() for t in (sdf, lap) if t is not None] or [0])
        for t, k in [(diff[0], 3 * n), (diff[1], 3 * n), (diff[2], 3 * n), (diff[3], n), (diff[4], n), (diff[5], n), (diff[6], n), (diff[7], n),
                     (rgb, 3 * n), (rgb_wo_mask, 3 * n), (alpha, n), (valid, n), (valid_phys, n), (sdf, m), (sdf_grad, 3 * m), (lap, m)]:
            if t is not None and t.numel() != k:
                raise L.IaError(f"fused training loss: an input has {t.numel()} elements where {k} are expected ({n} rays, {m} samples)")
        dev = next(t for t in diff + [rgb, rgb_wo_mask] if t is not None).device
        w = (C.c_float * N_TERMS)(*[float(x) for x in weights])
        terms, loss = torch.empty(N_TERMS, device=dev), torch.empty(1, device=dev)
        stats = torch.empty(N_STATS, dtype=torch.float64, device=dev)
        k = int(L.lib().ia_train_loss_partials(n, m))
        partials = torch.empty(max(k, 1), dtype=torch.float64, device=dev)
        L.lib().ia_train_loss(n, m, diff[0], diff[1], diff[2], diff[3], valid, valid_phys, rgb, rgb_wo_mask, alpha, diff[4], diff[5], diff[6],
                              diff[7], sdf, sdf_grad, lap, w, sparsity_scale, terms, loss, stats, partials)
        ctx.save_for_backward(*[t for t in diff[:4] + [sdf, sdf_grad, lap, rgb, rgb_wo_mask, alpha, valid, valid_phys, stats] if t is not None])
        ctx.present = [t is not None for t in diff[:4] + [sdf, sdf_grad, lap, rgb, rgb_wo_mask, alpha, valid, valid_phys, stats]]
        ctx.cfg = (n, m, tuple(float(x) for x in weights), float(sparsity_scale), shapes, dev)
        ctx.mark_non_differentiable(terms)
        ctx.set_materialize_grads(False)
        return loss[0], terms

    @staticmethod
    def backward(ctx, g_loss, _g_terms):
        n, m, weights, sparsity_scale, shapes, dev = ctx.cfg
        if g_loss is None:
            return (None,) * (_N_CONST + len(_DIFF))
        it = iter(ctx.saved_tensors)
        rgb_full, phys_full, demod_full, opacity, sdf, sdf_grad, lap, rgb, rgb_wo_mask, alpha, valid, valid_phys, stats = \
            [next(it) if p else None for p in ctx.present]
        inputs = dict(comp_rgb_full=rgb_full, comp_rgb_phys_full=phys_full, comp_demod_phys_full=demod_full, opacity=opacity,
                      sdf_samples=sdf, sdf_grad_samples=sdf_grad, sdf_laplace_samples=lap)
        grads = []
        for i, (name, deps) in enumerate(_DIFF):
            live = [k for k in deps if weights[k] != 0.0 and not (k in (6, 7) and alpha is None)]
            if name == "comp_rgb_full":
                live = live if rgb is not None else []
            elif name == "comp_rgb_phys_full":
                live = live if (rgb is not None or rgb_wo_mask is not None) else []
            elif name == "comp_demod_phys_full":
                live = live if rgb is not None else []
            want = shapes[i] is not None and ctx.needs_input_grad[_N_CONST + i] and bool(live) and (name in _MAPS or inputs[name] is not None)
            grads.append(torch.empty(shapes[i], device=dev) if want else None)
        w = (C.c_float * N_TERMS)(*weights)
        L.lib().ia_train_loss_bwd(n, m, rgb_full, phys_full, demod_full, opacity, valid, valid_phys, rgb, rgb_wo_mask, alpha, sdf, sdf_grad, lap, w,
                                  sparsity_scale, stats, g_loss.reshape(1).float().contiguous(), *grads)
        return (None,) * _N_CONST + tuple(grads)


def loss_weights(lam: Dict[str, float]):
    """the `lambda_*` entries of a (schedule-evaluated) `system.loss` dict in the kernel's term order; missing or None = 0"""
    w = [float(lam.get("lambda_" + k, 0.0) or 0.0) for k in TERMS]
    return w + [0.0] * (N_TERMS - len(w))


def fused_reference_loss(out: Dict[str, Tensor], rgb: Tensor, alpha: Optional[Tensor], lam: Dict[str, float], material,
                         rgb_wo_mask: Optional[Tensor] = None):
    """train_phys.reference_training_loss on the fused kernel: same arguments, same (loss, {term: value}) -- the terms a key of `out`
    or an argument is missing for are left out, as there (no `alpha`: no mask terms and no `opaque`) -- plus `curvature` when the dict
    has `sdf_laplace_samples`.  The term values are detached scalars (they are logged, not differentiated); `loss` carries the graph.
    `albedo_entropy` is evaluated only when its weight is not 0 (fields.albedo_entropy, as in VolumeMaterial.regularizations)."""
    g = out.get
    op = g("opacity") if alpha is not None else None
    loss, terms = _TrainLoss.apply(loss_weights(lam), float(lam.get("sparsity_scale", 1.0)), rgb, rgb_wo_mask, alpha, g("rays_valid_full"),
                                   g("rays_valid_phys_full"), g("comp_rgb_full"), g("comp_rgb_phys_full"), g("comp_demod_phys_full"), op,
                                   g(_MAPS[0]), g(_MAPS[1]), g(_MAPS[2]), g(_MAPS[3]), g("sdf_samples"), g("sdf_grad_samples"),
                                   g("sdf_laplace_samples"))
    need = dict(rgb_mse=("comp_rgb_full",), rgb_l1=("comp_rgb_full",), rgb_phys_mse=("comp_rgb_phys_full",), rgb_phys_l1=("comp_rgb_phys_full",),
                rgb_demodulated=("comp_demod_phys_full",), eikonal=("sdf_grad_samples",), mask_mse=("opacity",), mask_bce=("opacity",),
                opaque=("opacity",), sparsity=("sdf_samples",), curvature=("sdf_laplace_samples",), normal_orientation=(_MAPS[0],),
                albedo_smoothness=(_MAPS[1],), roughness_smoothness=(_MAPS[2],), metallic_smoothness=(_MAPS[3],))
    t = {}
    for k, name in enumerate(TERMS):
        if all(g(key) is not None for key in need[name]) and not (name in ("mask_mse", "mask_bce", "opaque") and alpha is None):
            t[name] = terms[k]
    w_ent = float(lam.get("lambda_albedo_entropy", 0.0) or 0.0)
    if w_ent != 0.0 and "comp_albedo_full" in out:
        t["albedo_entropy"] = fields.albedo_entropy(out["comp_albedo_full"][out["rays_valid_phys_full"][..., 0]])
        loss = loss + w_ent * t["albedo_entropy"]
    return loss, t
