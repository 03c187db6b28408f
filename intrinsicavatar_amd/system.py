"""The two callers either side of render_step ("adjacent step either side of the path"), host side:

    preprocess_data   systems/intrinsic_avatar.py:84-158    a dataset batch -> what the model is called with: rays [n,8] =
                                                            (o, d, near, far), the training targets composited over the step's
                                                            background colour (sRGB-encoded, as the images are), flat masks / maps
    chunk_batch       models/utils.py:16-61                 run a function over slices of its batched tensor arguments, merge the results
    model_forward     models/intrinsic_avatar.py:1653-1666  IntrinsicAvatarModel.forward: forward_ as it is in training, chunk_batch over
                                                            `ray_chunk` rays with the results moved to the host in evaluation, + "beta"
    evaluate_frame    systems/intrinsic_avatar.py:317-421,  the numeric part of validation_step / test_step: albedo-only pass -> ratio ->
                      :597-720                              relit pass, and the frame's metrics (metrics.py: kernels, results on the device;
                                                            the three *_lpips values on request, lpips=<metrics.LPIPSNet>)
    evaluate_sequence systems/intrinsic_avatar.py:597-720,  `mode=test` over a split with ground truth (data.TruthFrames): per frame the
                      models/intrinsic_avatar.py:281-305    pose / occupancy grid / emitter of `prepare`, then evaluate_frame
    mean_metrics      systems/intrinsic_avatar.py:869-911   test_epoch_end: the mean of every metric over the frames, one read-back

The first three are plain tensor plumbing on whatever device the batch lives on (no kernels: a few element-wise operators per frame); held to the reference's
own functions by tests/golden/golden_system.npz (tests/golden/make_golden_system.py)."""
from collections import defaultdict
from typing import Callable, Dict, Iterable, Iterator, Optional, Tuple

import torch
from torch import Tensor

from . import metrics, pbr

BACKGROUNDS = ("white", "black", "random")


def background_for(mode: str, stage: str, device, generator: Optional[torch.Generator] = None) -> Tensor:
    """the step's background colour (:121-143): the configured one while training, white otherwise."""
    if stage not in ("train",):
        return torch.ones(3, dtype=torch.float32, device=device)
    if mode == "white":
        return torch.ones(3, dtype=torch.float32, device=device)
    if mode == "black":
        return torch.zeros(3, dtype=torch.float32, device=device)
    if mode == "random":
        return torch.rand(3, dtype=torch.float32, device=device, generator=generator)
    raise NotImplementedError


def preprocess_data(batch: Dict[str, Tensor], stage: str, background_color: str = "white", device=None,
                    generator: Optional[torch.Generator] = None, background: Optional[Tensor] = None) -> Tuple[Dict[str, Tensor], Tensor, float]:
    """in place on `batch`, like the reference; -> (batch, background colour [3], t_idx).  `background`: an explicit colour instead of
    the draw of the "random" mode (parity with a recorded run)."""
    flat3 = lambda k: batch[k].reshape(-1, 3)      # noqa: E731
    if "hdri" in batch:
        assert stage in ["test"]
        assert batch["hdri"].shape[0] == 1
        batch["hdri"] = batch["hdri"].squeeze(0)
    rays = torch.cat([batch.pop("rays_o"), batch.pop("rays_d"), batch.pop("near")[..., None], batch.pop("far")[..., None]], dim=-1).reshape(-1, 8)
    batch["rays"] = rays
    dev = device if device is not None else rays.device
    bg = background.to(dev).float() if background is not None else background_for(background_color, stage, dev, generator)
    if "rgb" in batch:
        rgb = flat3("rgb")
        fg = batch["alpha"].reshape(-1)
        batch["rgb_wo_mask"] = rgb
        batch["rgb"] = rgb * fg[..., None] + pbr.rgb_to_srgb(bg.to(rgb.device) * (1 - fg[..., None]))
        batch["alpha"] = fg
    if "valid_mask" in batch:
        batch["valid_mask"] = batch["valid_mask"].reshape(-1)
    for k in ("albedo", "normal"):
        if k in batch:
            batch[k] = flat3(k)
    t_idx = batch["t_idx"] if stage in ["train"] else 0.0          # (not used in val / test / predict)
    return batch, bg, t_idx


def chunk_batch(func: Callable, chunk_size: int, move_to_cpu: bool, *args, **kwargs):
    """`func` on [i, i + chunk_size) of every positional tensor whose leading dimension equals that of the FIRST tensor argument; the
    chunks' results concatenated along dimension 0 -- a tensor, a tuple / list (type kept) or a dict of tensors; chunks that return None
    are left out, nothing returned at all gives None; results are detached when gradients are off and moved to the host on request."""
    B = next((a.shape[0] for a in args if isinstance(a, Tensor)), None)
    parts = defaultdict(list)
    kind, width = None, 0
    for i in range(0, B, chunk_size):
        r = func(*[a[i:i + chunk_size] if isinstance(a, Tensor) and a.shape[0] == B else a for a in args], **kwargs)
        if r is None:
            continue
        kind = type(r)
        if isinstance(r, Tensor):
            r = {0: r}
        elif isinstance(r, (tuple, list)):
            width = len(r)
            r = dict(enumerate(r))
        elif not isinstance(r, dict):
            raise TypeError(f"Return value of func must be in type [torch.Tensor, list, tuple, dict], get {type(r)}.")
        for k, v in r.items():
            v = v if torch.is_grad_enabled() else v.detach()
            parts[k].append(v.cpu() if move_to_cpu else v)
    if kind is None:
        return None
    merged = {k: torch.cat(v, dim=0) for k, v in parts.items()}
    if kind is Tensor:
        return merged[0]
    if kind in (tuple, list):
        return kind([merged[i] for i in range(width)])
    return merged


def model_forward(rs, rays: Tensor, material, emitter, spp: int, light_u: Tensor, shuffle_u: Optional[Tensor] = None, *, training: bool = False,
                  ray_chunk: int = 1 << 19, move_to_cpu: bool = True, **kw) -> Dict[str, Tensor]:
    """IntrinsicAvatarModel.forward (:1653-1666) over RenderStep: training -> forward_train_ on the whole batch; evaluation ->
    chunk_batch(forward_, ray_chunk, True, rays) -- every chunk's dict moved to the host and concatenated (per-ray maps along the rays,
    `num_samples*` as one entry per chunk, like the reference's) -- and the density's beta added.  The light directions (light_u [spp,3])
    are shared by the chunks; shuffle_u [n,spp] is sliced with the rays."""
    if training:
        out = rs.forward_train_(rays, material, emitter, spp, light_u, shuffle_u=shuffle_u, **kw)
    elif shuffle_u is None:
        out = chunk_batch(lambda r: rs.forward_(r, material, emitter, spp, light_u, None, **kw), ray_chunk, move_to_cpu, rays)
    else:
        out = chunk_batch(lambda r, su: rs.forward_(r, material, emitter, spp, light_u, su, **kw), ray_chunk, move_to_cpu, rays, shuffle_u)
    return {**out, "beta": rs.density.get_beta()}


METRIC_KEYS = ("rf_psnr", "rf_ssim", "normal_error", "pbr_psnr", "pbr_ssim", "albedo_psnr", "albedo_ssim")      # the reference's, minus *_lpips
LPIPS_KEYS = ("rf_lpips", "pbr_lpips", "albedo_lpips")                # ... which a call with lpips=<metrics.LPIPSNet> adds


def evaluate_frame(rs, batch: Dict[str, Tensor], material, emitter, spp: int, light_u: Tensor, shuffle_u: Optional[Tensor] = None, *,
                   img_wh: Tuple[int, int], stage: str = "test", lpips=None, **kw) -> Tuple[Dict[str, Tensor], Dict[str, Tensor]]:
    """the numeric part of validation_step (:317-421) / test_step (:597-720) on a batch that went through preprocess_data (device
    tensors).  stage "test" with both "hdri" and "albedo" in the batch: an albedo-only pass, the per-channel ratio against the ground
    truth, then the full pass with that ratio (its comp_albedo_full IS the aligned albedo, :697-698); otherwise one full pass and, if
    "albedo" is there, the alignment afterwards (:380-399, :681-696).  -> (metrics, out): metrics under the reference's keys without
    *_lpips, 0-d device tensors (metrics.to_host(metrics): every one of them with a single read-back); out = the model's dict on the
    device with "comp_normal" in OpenGL camera space, + "aligned_albedo" when one was formed.  lpips: a metrics.LPIPSNet adds the
    reference's rf_lpips / pbr_lpips (valid_mask's rectangle) and albedo_lpips (gt_mask's), each under the condition of the SSIM next to
    it and equal to metrics.LPIPS()(prediction, target, lpips, valid_mask) bit for bit; five images go through the trunk, in two
    batches.  **kw goes to model_forward."""
    assert stage in ("validation", "test")
    W, H = img_wh
    rays = batch["rays"]
    kw = dict(kw, move_to_cpu=False)
    aligned_by_model = stage == "test" and "hdri" in batch and "albedo" in batch
    gt_albedo = batch.get("albedo")
    gt_mask = batch["alpha"] > 0.5 if ("albedo" in batch or "normal" in batch) else None
    ratio = None
    if aligned_by_model:
        pred_albedo = model_forward(rs, rays, material, emitter, spp, light_u, shuffle_u, albedo_only=True, **kw)["comp_albedo_full"]
        ratio = metrics.compute_albedo_rescale_factor(gt_albedo, pred_albedo, gt_mask)
    out = model_forward(rs, rays, material, emitter, spp, light_u, shuffle_u, albedo_align_ratio=ratio, **kw)
    valid = batch.get("valid_mask")
    psnr, ssim = metrics.PSNR(), metrics.SSIM()
    img = lambda t: t.reshape(H, W, 3)      # noqa: E731
    ret = {}
    if "rgb" in batch:
        rect = metrics.mask_rect(valid.reshape(H, W)) if valid is not None else None
        ret["rf_psnr"] = psnr(out["comp_rgb_full"], batch["rgb"], valid_mask=valid)
        ret["rf_ssim"] = metrics.ssim(img(out["comp_rgb_full"]), img(batch["rgb"]), rect)
        if lpips is not None:
            # (one batch of three through the trunk: the target once, and three times the workgroups in the deep layers)
            feats = metrics.lpips_features(lpips, [img(out["comp_rgb_full"]), img(out["comp_rgb_phys_full"]), img(batch["rgb"])], rect)
            ret["rf_lpips"] = metrics.lpips_of_features(lpips, feats, feats, rect, slots=(0, 2))
    if "normal" in batch:
        r = metrics.normal_error(out["comp_normal"], batch["normal"], gt_mask, w2c=batch.get("w2c"), transform=True, normalize=True,
                                 want_camera=True)
        out["comp_normal"] = r["camera"]
        ret["normal_error"] = r["mean"]
    else:
        out["comp_normal"] = metrics.transform_normals(out["comp_normal"], batch.get("w2c"))
    if "rgb" in batch:
        ret["pbr_psnr"] = psnr(out["comp_rgb_phys_full"], batch["rgb"], valid_mask=valid)
        ret["pbr_ssim"] = metrics.ssim(img(out["comp_rgb_phys_full"]), img(batch["rgb"]), rect)
        if lpips is not None:
            ret["pbr_lpips"] = metrics.lpips_of_features(lpips, feats, feats, rect, slots=(1, 2))
    if "albedo" in batch:
        if aligned_by_model:
            aligned = out["comp_albedo_full"]
        else:
            aligned, ratio = metrics.align_albedo(gt_albedo, out["comp_albedo_full"], gt_mask)
        out["aligned_albedo"] = aligned
        ret["albedo_psnr"] = psnr(aligned, gt_albedo, valid_mask=gt_mask)
        ret["albedo_ssim"] = ssim(img(aligned), img(gt_albedo), valid_mask=gt_mask.reshape(H, W))
        if lpips is not None:
            grect = metrics.mask_rect(gt_mask.reshape(H, W))
            feats = metrics.lpips_features(lpips, [img(aligned), img(gt_albedo)], grect)
            ret["albedo_lpips"] = metrics.lpips_of_features(lpips, feats, feats, grect, slots=(0, 1))
    return ret, out


def evaluate_sequence(rs, material, frames, body, spp: int, *, stage: str = "test", emitter=None, render_mode: str = "light",
                      global_illumination: bool = True, resample_light: bool = True, generator: Optional[torch.Generator] = None,
                      frames_idx: Optional[Iterable[int]] = None, cano_pose="da_pose", occ_res: int = 64,
                      ray_chunk: int = 1 << 19, lpips=None) -> Iterator[Tuple[int, Dict[str, Tensor], Dict[str, Tensor]]]:
    """the reference's `mode=test` over a split with ground truth: yields (idx, metrics, out) per frame of data.TruthFrames -- full_frame
    -> animation.prepare_frame (pose, bbox, test occupancy grid, as render_sequence) -> preprocess_data(stage) -> evaluate_frame with
    img_wh = frames.img_wh.  `out` also carries the random tensors it was made with (`light_u`, `shuffle_u`), drawn from `generator` in
    render_sequence's order.  emitter: given, or an EnvironmentLightTensor of the frame's "hdri", rebuilt (with update_pdf) only when
    that tensor changes (IntrinsicAvatarModel.prepare, models/intrinsic_avatar.py:286-305); resample_light=False draws light_u once.
    lpips: a metrics.LPIPSNet for the three *_lpips values (evaluate_frame).  mean_metrics(list of the yielded metrics) is test_epoch_end."""
    from . import animation, smpl                                   # (animation imports this module)
    if render_mode in ("mats", "mis"):
        raise NotImplementedError("evaluate_sequence draws the random tensors of the light / uniform_light estimators")
    dev = rs.deformer.device
    dt = body.v_template.dtype
    rest = body.forward(frames.betas[:1].to(dt), smpl.rest_pose(cano_pose, device=body.v_template.device).to(dt),
                        torch.zeros((1, 3), dtype=dt, device=body.v_template.device))
    A_rest_inv = torch.linalg.inv(rest["A"].float())
    n_light = 512 if render_mode == "uniform_light" else spp
    given, built_from, light_u = emitter, None, None
    for idx in (range(len(frames)) if frames_idx is None else frames_idx):
        batch = dict(frames.full_frame(idx))
        batch.pop("pixel_indices", None)
        batch.pop("status", None)
        occ_rand = animation._rand((occ_res ** 3, 3, 3), dev, generator)
        animation.prepare_frame(rs, body, A_rest_inv, batch, occ_rand, occ_res)
        batch, bg, _ = preprocess_data(batch, stage)
        if given is None:
            if "hdri" not in batch:
                raise ValueError("evaluate_sequence needs an emitter or frames whose full_frame carries an HDRI (the test split)")
            if built_from is None or built_from.data_ptr() != batch["hdri"].data_ptr() or built_from.shape != batch["hdri"].shape:
                built_from = batch["hdri"]
                emitter = pbr.EnvironmentLightTensor(built_from.contiguous())
                emitter.update_pdf()
        rays = batch["rays"]
        if light_u is None or resample_light:
            light_u = animation._rand((n_light, 3), dev, generator)
        shuffle_u = animation._rand((rays.shape[0], spp), dev, generator)
        ret, out = evaluate_frame(rs, batch, material, emitter, spp, light_u, shuffle_u, img_wh=frames.img_wh, stage=stage, background_color=bg,
                                  global_illumination=global_illumination, render_mode=render_mode, ray_chunk=ray_chunk, lpips=lpips)
        out["light_u"], out["shuffle_u"] = light_u, shuffle_u
        yield int(idx), ret, out


def mean_metrics(per_frame) -> Dict[str, float]:
    """test_epoch_end (systems/intrinsic_avatar.py:905-911): the mean of every metric over the frames, formed on the device (float64) and
    read back with ONE copy for all keys; ValueError if a frame's metric could not be formed (metrics.to_host's statuses)."""
    per_frame = list(per_frame)
    if not per_frame:
        return {}
    keys = list(per_frame[0])
    plain = lambda t: t.as_subclass(Tensor).double().reshape(-1)      # noqa: E731
    means = [torch.stack([plain(m[k])[0] for m in per_frame]).mean() for k in keys]
    bufs = [(k, m[k]._buf) for m in per_frame for k in keys if getattr(m[k], "_buf", None) is not None]
    host = torch.cat([torch.stack(means)] + [plain(b)[-1:] for _, b in bufs]).cpu()
    for (k, _), status in zip(bufs, host[len(keys):].tolist()):
        metrics._raise_on_status(int(status), k)
    return {k: float(v) for k, v in zip(keys, host[:len(keys)].tolist())}
