"""The reference's animation / relighting test path (`mode=test dataset=animation/...`): a trained avatar driven by a motion, lit by an
HDRI and -- with add_emitter -- shown in that environment.

    render_sequence(rs, material, frames, body, spp, ...)    generator of (idx, out_dict), one per frame of data.AnimationFrames
    save_frame(out, H, W, path_prefix)                       the reference's per-frame panels (systems/intrinsic_avatar.py:723-850)

Per frame (IntrinsicAvatarModel.prepare, models/intrinsic_avatar.py:281-305; test_step, systems/intrinsic_avatar.py:597-720):
SMPL kinematics -> bone transforms in the SMPL-root frame -> deformer.prepare -> the canonical bbox to the geometry / radiance fields ->
the test occupancy grid over the bbox of the posed vertices (:307-381) -> preprocess_data(stage="test") -> model_forward.  The emitter is
an EnvironmentLightTensor of the frames' HDRI, built once (the reference re-assigns the same image every frame it re-samples).
resample_light (configs/config.yaml:56, :288-305): True draws the spp light directions once per frame; False ("for generating
animation") once for the sequence -- identical WORLD directions, rotated into each frame's SMPL space by emitter.sample(..., w2s_rot).
"""
from typing import Dict, Iterable, Iterator, Optional, Tuple

import torch
from torch import Tensor

from . import io_formats, occ_grid, pbr, render, smpl, system


def _rand(shape, device, generator):
    """uniforms on `device` from `generator` (a generator of that device or of the CPU; None: the device's default)"""
    if generator is not None and generator.device.type != torch.device(device).type:
        return torch.rand(shape, generator=generator).to(device)
    return torch.rand(shape, device=device, generator=generator)


@torch.no_grad()
def prepare_frame(rs, body, A_rest_inv: Tensor, batch: Dict[str, Tensor], occ_rand: Optional[Tensor] = None, occ_res: int = 64) -> None:
    """IntrinsicAvatarModel.prepare in eval mode, on `rs` in place: pose the body, hand the bone transforms to the deformer, give the
    canonical bbox to both fields and build the frame's occupancy grid from the model.  occ_rand [occ_res^3, 3, 3]: the jitter."""
    dfm = rs.deformer
    dev = dfm.device
    dt = body.v_template.dtype
    out = body.forward(batch["betas"].to(dt), batch["body_pose"].to(dt), batch["global_orient"].to(dt), batch["transl"].to(dt))
    tfs, w2s = smpl.deformer_transforms(out["A"], A_rest_inv)
    dfm.prepare(tfs, w2s[0])
    rs.geometry.prepare_bbox(dfm.bbox)
    rs.radiance.prepare_bbox(dfm.bbox)
    # deformed bbox: get_bbox_from_smpl of the vertices in SMPL space (snarf_deformer.py:113-115, intrinsic_avatar.py:309)
    verts = out["vertices"].float() @ w2s[:, :3, :3].permute(0, 2, 1) + w2s[:, None, :3, 3]
    aabb = smpl.bbox_from_vertices(verts).reshape(-1).to(dev)
    beta_t = rs.density.get_beta().detach().reshape(1)
    step = rs.render_step_size

    def occ_eval_fn(x):
        return render.laplace_alpha(dfm.deform(x, rs.geometry)["sdf"], step, beta_t)

    _, binaries = occ_grid.compute_test_occupancy_grid(occ_eval_fn, aabb, occ_res, 3, 0.01, occ_rand)
    rs.binaries, rs.aabbs = binaries.contiguous(), aabb[None].contiguous()
    # the render step keys its cached forms of the grid by (address, version): a new frame's tensors may land at the old address
    rs._grid_bits = None
    rs._sort_grid_cache = None


def render_sequence(rs, material, frames, body, spp: int, *, add_emitter: bool = False, resample_light: bool = True,
                    render_mode: str = "light", global_illumination: bool = True, generator: Optional[torch.Generator] = None,
                    ray_chunk: int = 1 << 19, frames_idx: Optional[Iterable[int]] = None, cano_pose="da_pose", occ_res: int = 64,
                    emitter=None) -> Iterator[Tuple[int, Dict[str, Tensor]]]:
    """relit frames of a motion: yields (idx, out) with `out` the model's dict on the device (model_forward, move_to_cpu=False) plus the
    random tensors it was made with (`light_u` [spp,3], `shuffle_u` [n_rays,spp]).
    frames: data.AnimationFrames; body: smpl.SMPLKinematics of the subject; emitter: default = EnvironmentLightTensor of the frames'
    HDRI (required then).  add_emitter: the environment behind the avatar (RenderStep.relight).  generator: all random tensors."""
    dev = rs.deformer.device
    if emitter is None:
        if frames.hdri is None:
            raise ValueError("render_sequence needs an emitter or frames with an HDRI (AnimationFrames.from_dir(..., hdri_filepath=...))")
        emitter = pbr.EnvironmentLightTensor(frames.hdri[0].contiguous())
        emitter.update_pdf()
    dt = body.v_template.dtype
    rest = body.forward(frames.betas[:1].to(dt), smpl.rest_pose(cano_pose, device=body.v_template.device).to(dt),
                        torch.zeros((1, 3), dtype=dt, device=body.v_template.device))
    A_rest_inv = torch.linalg.inv(rest["A"].float())
    n_light = 512 if render_mode == "uniform_light" else spp
    light_u = None
    for idx in (range(len(frames)) if frames_idx is None else frames_idx):
        batch = dict(frames.frame(idx))
        occ_rand = _rand((occ_res ** 3, 3, 3), dev, generator)
        prepare_frame(rs, body, A_rest_inv, batch, occ_rand, occ_res)
        batch, bg, _ = system.preprocess_data(batch, "test")
        rays = batch["rays"]
        if light_u is None or resample_light:
            light_u = _rand((n_light, 3), dev, generator)
        shuffle_u = _rand((rays.shape[0], spp), dev, generator) if render_mode in ("light", "uniform_light") else None
        kw = dict(background_color=bg, global_illumination=global_illumination, render_mode=render_mode, add_emitter=add_emitter)
        if render_mode in ("mats", "mis"):
            raise NotImplementedError("render_sequence draws the random tensors of the light / uniform_light estimators")
        out = system.model_forward(rs, rays, material, emitter, spp, light_u, shuffle_u, ray_chunk=ray_chunk, move_to_cpu=False, **kw)
        out["light_u"], out["shuffle_u"] = light_u, shuffle_u
        yield int(idx), out


def save_frame(out: Dict[str, Tensor], H: int, W: int, path_prefix: str) -> Dict[str, str]:
    """the panels test_step writes for a frame without ground truth (systems/intrinsic_avatar.py:723-850): `<prefix>.png`, the grid
    rf_rgb | pbr_rgb | pbr_demod | pbr_albedo | pbr_metallic | pbr_roughness [| visibility] | depth | normal, and every panel on its own
    as `<prefix>-<caption>.png`.  -> {caption: path}."""
    from PIL import Image
    rgb = lambda k, **kw: {"type": "rgb", "img": out[k].reshape(H, W, 3), "kwargs": dict({"data_format": "HWC"}, **kw)}      # noqa: E731
    gray = lambda k, **kw: {"type": "grayscale", "img": out[k].reshape(H, W), "kwargs": kw}                                  # noqa: E731
    panels = [("rf_rgb", rgb("comp_rgb_full")), ("pbr_rgb", rgb("comp_rgb_phys_full")), ("pbr_demod", rgb("comp_demod_phys_full")),
              ("pbr_albedo", rgb("comp_albedo_full")), ("pbr_metallic", gray("comp_metallic_full", data_range=(0, 1), cmap=None)),
              ("pbr_roughness", gray("comp_roughness_full", data_range=(0, 1), cmap=None))]
    if "visibility" in out:
        panels.append(("visibility", gray("visibility", data_range=(0, 1), cmap=None)))
    panels += [("depth", gray("depth")), ("normal", rgb("comp_normal", data_range=(-1, 1)))]
    io_formats.save_image_grid(path_prefix + ".png", [p for _, p in panels])
    paths = {"grid": path_prefix + ".png"}
    for caption, p in panels:
        paths[caption] = f"{path_prefix}-{caption}.png"
        Image.fromarray(io_formats.image_grid_u8([p])).save(paths[caption])
    return paths
