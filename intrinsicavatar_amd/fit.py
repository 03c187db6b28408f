"""The training run: what the reference spreads over BaseSystem.on_train_batch_start (systems/base.py:109-135),
IntrinsicAvatarModel.update_step (models/intrinsic_avatar.py:224-275), IntrinsicAvatarSystem.training_step
(systems/intrinsic_avatar.py:160-301) and reinit_occupancy_grid (:46-79), on the pieces of this package.

    Schedule     BaseSystem.C (systems/base.py:33-88) and the switches that depend on the step
    FitConfig    the `model`, `system.loss`, `trainer` (and the scalar `system` / optimiser) values of configs/config.yaml
    Trainer      one frame per step: batch -> pose -> grid -> forward -> fused loss -> backward -> Adam -> LR schedule

Pose correction (Trainer(..., pose_correction=pose_correction.PoseCorrection(...)), config.enable_pose_correction): order within a
step as in systems/base.py:109-111 -- the frame is posed with the module's switch as the PREVIOUS step left it, only then does
update_step(epoch, global_step) run.  update_step turns the switch on when global_step > pose_correction_start_step = S, i.e. during
step S + 1, after that step's pose: the first step that adds corrections has global_step = S + 2.  From then on the step's
body_pose / global_orient / transl are the dataset's plus the frame's rows, SMPL kinematics run with grad, the deformer is prepared
with the differentiable tfs and the DETACHED w2s (snarf_deformer.py:130,148,156), and the grid update and reinit_grids pose every
frame with its corrected parameters under no_grad.  betas_correction is carried in the state dict and never added (optimize_betas: false).

Random numbers: EVERY random tensor of a step comes from the Trainer's one generator, drawn at the top of step() in this order
(a tensor that the step's phase does not use is not drawn), and is returned in the step's record so that the step can be replayed:

    perm          [F] int64          torch.randperm, once per epoch (the reference's DataLoader(shuffle=True)), at the epoch's first step
    words         [n_rays] int64     the pixel sampler's words (data.TrainingFrames.batch)
    background    [3]                model.background_color == "random"
    jitter        [n_rays]           model.randomized: stratified near plane
    curv_u        [cap, 3]           with_curvature: curvature probe directions (uniform)
    material_jitter [cap, 3]         enable_phys and jitter_materials: standard normal
    light_u       [512, 3] (uniform_light) or [n_rays * spp, 3] (light: one direction per foreground point)      enable_phys
    shuffle_u     [n_rays, spp]      enable_phys, uniform_light
    grid_rand     [res^3, 3]         grid_update: jitter of the occupancy update
    reinit_rand   [F, res^3, 3, 3]   reinit_grid: jitter of every frame's grid
cap = n_rays * (num_samples_per_ray + 40) rows: the per-sample tensors are drawn before the march has counted the samples (a ray
crosses the scene box in at most num_samples_per_ray steps and each of the two importance passes adds 16); the forward reads the
first n_samples rows and the record keeps those.

Deviations from the reference, all at the grid re-initialisation step: the reference's reinit_occupancy_grid leaves the model posed
as the LAST frame of the dataset (and with that frame's t_idx) for the training step that follows; here the step's own frame is
posed again.  The reference also draws a background colour per frame while it walks the dataset; nothing reads it, none is drawn.
"""
import copy
import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import torch
from torch import Tensor

from . import checkpoint, occ_grid, optim, render, smpl, system, train_loss


def _model_defaults():
    return dict(name="intrinsic-avatar", global_illumination=True, render_mode="uniform_light", samples_per_pixel=512,
                num_samples_per_ray=128, num_samples_per_secondary_ray=64, secondary_shader_chunk=160000, secondary_near_plane=0.0,
                secondary_far_plane=1.5, secondary_importance_sample=True, zero_crossing_search=True, resample_light=True,
                volume_scattering=True, add_emitter=False, grid_prune=True, grid_prune_occ_thre=0.001, grid_prune_ema_decay=0.8,
                randomized=True, ray_chunk=4096, learned_background=False, learn_material=True, material_feature="hybrid",
                phys_kick_in_step=10000, importance_sample_kick_in_step=1000, background_color="random")


def _loss_defaults():
    return dict(lambda_rgb_l1=1.0, lambda_rgb_phys_l1=0.2, lambda_mask_bce=0.1, lambda_eikonal=0.1,
                lambda_lipshitz_bound=[12500, 1.0e-5, 1.0e-5, 12501], lambda_curvature=[1.5, 0.0, 12500], lambda_albedo_smoothness=0.01,
                lambda_roughness_smoothness=0.01, lambda_metallic_smoothness=0.01, sparsity_scale=1.0, lambda_rgb_mse=0.0,
                lambda_rgb_phys_mse=0.0, lambda_rgb_demodulated=0.0, lambda_mask_mse=0.0, lambda_sparsity=0.0, lambda_distortion=0.0,
                lambda_opaque=0.0, lambda_albedo=0.0, lambda_normal_orientation=0.0, lambda_albedo_entropy=0.0,
                lambda_energy_conservation=0.0)


def _trainer_defaults():
    return dict(max_steps=25000, log_every_n_steps=100, num_sanity_val_steps=0, val_check_interval=2000, check_val_every_n_epoch=None,
                limit_train_batches=1.0, limit_val_batches=2, enable_progress_bar=True, precision=32)


def _system_defaults():
    return dict(name="intrinsic-avatar-system", pbr_loss_only=False,reinit_occupancy_grid_steps=[8000], reinit_shape_every_n_steps=-1, warmup_steps=1000)


def _optimizer_defaults():
    return dict(lr=0.001, betas=[0.9, 0.99], eps=1.0e-15, color_grid_wd=0.0001, milestones=[12500, 18750, 22500, 23750], gamma=0.3)


@dataclass
class FitConfig:
    """configs/config.yaml: `model` (its scalar entries; the `${...}` references to other config groups are the objects a Trainer is
    built from), `system.loss`, `trainer`, the scalar entries of `system`, and the optimiser / scheduler numbers.  What the reference
    hard-codes or keeps in other files follows: the grid update period (models/intrinsic_avatar.py:263), the grid resolution (:203),
    the dataset's scene box (configs/dataset/peoplesnapshot/*.yaml), the canonical pose and the options that are out of scope."""
    model: Dict = field(default_factory=_model_defaults)
    loss: Dict = field(default_factory=_loss_defaults)
    trainer: Dict = field(default_factory=_trainer_defaults)
    system: Dict = field(default_factory=_system_defaults)
    optimizer: Dict = field(default_factory=_optimizer_defaults)
    grid_update_every: int = 20
    grid_resolution: int = 64
    scene_aabb: List[float] = field(default_factory=lambda: [-1.25, -1.55, -1.25, 1.25, 0.95, 1.25])
    cano_pose: object = "da_pose"
    enable_pose_correction: bool = False
    pose_correction_start_step: int = 4000
    pose_correction_wd: float = 1e-5
    optimize_betas: bool = False
    reinit_optimizer_steps: List[int] = field(default_factory=list)
    world_size: int = 1

    def check_scope(self, pose_correction=None) -> None:
        """raises NotImplementedError for what this driver does not do; pose_correction: the module the Trainer was given"""
        def positive(v):
            return any(float(x) > 0 for x in (v[-3:-1] if isinstance(v, (list, tuple)) else [v or 0.0]))
        bad = []
        if self.enable_pose_correction and pose_correction is None:
            bad.append("enable_pose_correction: needs a module (Trainer(..., pose_correction=pose_correction.PoseCorrection(...)))")
        if self.optimize_betas:
            bad.append("optimize_betas: SMPL shape optimisation is outside the render-step path")
        if int(self.system.get("reinit_shape_every_n_steps", -1) or -1) > 0:
            bad.append("reinit_shape_every_n_steps > 0: belongs to SMPL shape optimisation")
        if [s for s in self.reinit_optimizer_steps if int(s) >= 0]:
            bad.append("reinit_optimizer_steps: the optimiser is built once")
        if self.system.get("pbr_loss_only"):
            bad.append("pbr_loss_only: ablation switch of the reference, not built")
        if positive(self.loss.get("lambda_distortion", 0.0)):
            bad.append("lambda_distortion > 0: the distortion loss has no kernel")
        if positive(self.loss.get("lambda_albedo", 0.0)):
            bad.append("lambda_albedo > 0: needs ground-truth albedo in the training batch")
        if self.model.get("learned_background"):
            bad.append("learned_background: not implemented in the reference either")
        if int(self.world_size) != 1:
            bad.append("world_size > 1: the driver runs on one GPU (parallel.py holds the multi-GPU pieces)")
        if not self.model.get("grid_prune", True):
            bad.append("grid_prune = false: the march needs the occupancy grid")
        if self.model.get("render_mode") not in ("uniform_light", "light"):
            bad.append(f"render_mode {self.model.get('render_mode')!r}: the driver draws the random tensors of light / uniform_light")
        if bad:
            raise NotImplementedError("fit.Trainer: out of scope -- " + "; ".join(bad))


@dataclass
class Phase:
    """what the schedule demands at one step"""
    global_step: int
    epoch: int
    enable_phys: bool
    importance_sample: bool
    with_curvature: bool
    jitter_materials: bool
    lam: Dict[str, float]
    grid_update: bool
    reinit_grid: bool


class Schedule:
    def __init__(self, config: Optional[FitConfig] = None):
        self.config = config if config is not None else FitConfig()

    @staticmethod
    def C(value, global_step: int, epoch: int):
        """BaseSystem.C: a number is itself; [start_value, end_value, end_step] switches at end_step; [start_step, start_value,
        end_value, end_step] is 0 before start_step, then ramps linearly to end_value at end_step.  An int end_step counts global
        steps, a float end_step counts epochs."""
        if isinstance(value, (int, float)):
            return value
        if not isinstance(value, (list, tuple)):
            raise TypeError(f"Scalar specification only supports list, got {type(value)}")
        if len(value) not in (3, 4):
            raise AssertionError("a schedule is a list of 3 or 4 entries")
        end_step = value[-1]
        if isinstance(end_step, int):
            now = global_step
        elif isinstance(end_step, float):
            now = epoch
        else:
            return list(value)          # the reference leaves such a list as it is
        if len(value) == 3:
            start_value, end_value, _ = value
            return start_value if now < end_step else end_value
        start_step, start_value, end_value, _ = value
        if now < start_step:
            return 0.0
        return start_value + (end_value - start_value) * max(min(1.0, (now - start_step) / (end_step - start_step)), 0.0)

    def at(self, global_step: int, epoch: int = 0) -> Phase:
        cfg = self.config
        lam = {k: self.C(v, global_step, epoch) for k, v in cfg.loss.items() if k.startswith("lambda_")}
        return Phase(global_step=int(global_step), epoch=int(epoch),
                     enable_phys=global_step >= cfg.model.get("phys_kick_in_step", 10000),
                     importance_sample=global_step > cfg.model.get("importance_sample_kick_in_step", 1000),
                     with_curvature=lam.get("lambda_curvature", 0.0) > 0,
                     jitter_materials=lam.get("lambda_albedo_smoothness", 0.0) > 0,
                     lam=lam, grid_update=global_step % int(cfg.grid_update_every) == 0,
                     reinit_grid=global_step in list(cfg.system.get("reinit_occupancy_grid_steps", [-1])))


_MAP_TERMS = ("normal_orientation", "albedo_smoothness", "roughness_smoothness", "metallic_smoothness")
_SAMPLE_SLACK = 40          # samples per ray beyond num_samples_per_ray that the per-sample random tensors are drawn for


class Trainer:
    """rs: render.RenderStep (geometry, radiance, density, deformer); material: fields.VolumeMaterial; emitter: a pbr.EnvironmentLight*;
    frames: data.TrainingFrames / TruthFrames with a sampler; body: smpl.SMPLKinematics; generator: the one source of random numbers
    (of the frames' device, or of the CPU: then every draw is made on the host and copied); pose_correction: a
    pose_correction.PoseCorrection with one row per frame (moved to the frames' device), or None: the dataset's SMPL fits as they are.
    The module's own enable flag and start step are the ones it was built with; the config's say whether a module is expected."""

    def __init__(self, rs, material, emitter, frames, body, config: Optional[FitConfig] = None, generator: Optional[torch.Generator] = None,
                 pose_correction=None):
        self.config = config if config is not None else FitConfig()
        self.config.check_scope(pose_correction)
        if frames.sampler is None:
            raise ValueError("fit.Trainer needs frames with a pixel sampler")
        self.rs, self.material, self.emitter, self.frames, self.body = rs, material, emitter, frames, body
        self.device = frames.device
        self.pose_correction = pose_correction.to(self.device) if pose_correction is not None else None
        if self.pose_correction is not None and self.pose_correction.dataset_length != len(frames):
            raise ValueError(f"pose_correction has {self.pose_correction.dataset_length} rows for {len(frames)} frames")
        self.generator = generator if generator is not None else torch.Generator(device=self.device)
        self.schedule = Schedule(self.config)
        oc, sc = self.config.optimizer, self.config.system
        self.optimizer, self.scheduler = optim.reference_optimizer(rs, lr=oc["lr"], color_grid_wd=oc["color_grid_wd"], material=material,
                                                                   emitter=emitter, warmup_steps=sc["warmup_steps"],
                                                                   milestones=tuple(oc["milestones"]), gamma=oc["gamma"],
                                                                   pose_correction=self.pose_correction,
                                                                   pose_correction_wd=float(self.config.pose_correction_wd))
        for g in self.optimizer.param_groups:
            g["betas"], g["eps"] = tuple(oc["betas"]), oc["eps"]
        self.grid = self._new_grid(torch.tensor(self.config.scene_aabb, dtype=torch.float32).reshape(1, 6), 1)
        dt = body.v_template.dtype
        rest = body.forward(frames.betas[:1].to(dt), smpl.rest_pose(self.config.cano_pose, device=body.v_template.device).to(dt),
                            torch.zeros((1, 3), dtype=dt, device=body.v_template.device))
        self.A_rest_inv = torch.linalg.inv(rest["A"].float())
        self.n_rays = int(frames.sampler.num_sample)
        self.sample_cap = self.n_rays * (int(self.config.model["num_samples_per_ray"]) + _SAMPLE_SLACK)
        self.global_step, self.epoch = 0, 0
        self._perm, self._pos = None, 0

    # ------------------------------------------------------------------ random numbers
    def _draw(self, kind: str, *shape) -> Tensor:
        g = self.generator
        if kind == "perm":
            t = torch.randperm(shape[0], generator=g, device=g.device)
        elif kind == "words":
            t = torch.randint(0, 2 ** 63 - 1, shape, dtype=torch.int64, generator=g, device=g.device)
        elif kind == "normal":
            t = torch.randn(shape, generator=g, device=g.device)
        else:
            t = torch.rand(shape, generator=g, device=g.device)
        return t.to(self.device)

    # ------------------------------------------------------------------ pose and grids
    def _new_grid(self, aabbs: Tensor, levels: int):
        grid = occ_grid.TemporalOccGridEstimator(aabbs, int(self.config.grid_resolution), levels=levels).to(self.device)
        grid.train()
        return grid

    def pose(self, params: Dict[str, Tensor]) -> Tensor:
        """animation.prepare_frame without its occupancy grid: SMPL kinematics -> deformer.prepare -> canonical bbox to both fields.
        -> the box of the posed vertices in SMPL space [6] (get_bbox_from_smpl).  Parameters that carry a graph (corrected_params
        with the switch on, grad mode on) leave a deformer whose tfs requires grad; w2s is detached either way."""
        rs, body, dfm = self.rs, self.body, self.rs.deformer
        dt = body.v_template.dtype
        with torch.set_grad_enabled(torch.is_grad_enabled() and any(v.requires_grad for v in params.values())):
            out = body.forward(params["betas"].to(dt), params["body_pose"].to(dt), params["global_orient"].to(dt), params["transl"].to(dt))
            tfs, w2s = smpl.deformer_transforms(out["A"], self.A_rest_inv)
        w2s = w2s.detach()
        dfm.prepare(tfs, w2s[0])
        with torch.no_grad():
            rs.geometry.prepare_bbox(dfm.bbox)
            rs.radiance.prepare_bbox(dfm.bbox)
            verts = out["vertices"].float() @ w2s[:, :3, :3].permute(0, 2, 1) + w2s[:, None, :3, 3]
            return smpl.bbox_from_vertices(verts).reshape(-1).to(self.device)

    def corrected_params(self, idx: int, params: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
        """frame idx's SMPL parameters (`params`, or the dataset's) plus the module's rows: body_pose, global_orient and transl;
        betas stay the dataset's.  Without a module, or while its switch is off, `params` as they are (nothing is added, not even
        zeros: the step is bit-identical to one without the module)."""
        params = params if params is not None else self._frame_params(idx)
        pc = self.pose_correction
        if pc is None or not pc.enable_pose_correction:
            return params
        c = pc(torch.tensor([idx], dtype=torch.int64, device=self.device))
        return dict(betas=params["betas"], body_pose=params["body_pose"] + c["pose_correction"].to(params["body_pose"].dtype),
                    global_orient=params["global_orient"] + c["global_orient_correction"].to(params["global_orient"].dtype),
                    transl=params["transl"] + c["transl_correction"].to(params["transl"].dtype))

    def occ_eval_fn(self) -> Callable:
        """alpha of one render step at posed-space points: the occ_eval_fn of animation.prepare_frame"""
        rs = self.rs
        beta_t = rs.density.get_beta().detach().reshape(1)
        step = rs.render_step_size

        def fn(x):
            return render.laplace_alpha(rs.deformer.deform(x, rs.geometry)["sdf"], step, beta_t)
        return fn

    def _frame_params(self, idx: int) -> Dict[str, Tensor]:
        f, s = self.frames, slice(idx, idx + 1)
        return dict(betas=f.betas, body_pose=f.body_pose[s], global_orient=f.global_orient[s], transl=f.transl[s])

    @torch.no_grad()
    def reinit_grids(self, rand: Optional[Tensor] = None) -> Tensor:
        """reinit_occupancy_grid: every training frame in dataset order gets the grid of prepare_test_occupancy_grid (64^3 cells over the
        box of its posed vertices, 3 jittered samples per cell, grid_prune_occ_thre), stacked into an estimator with one level per
        frame.  rand [F, res^3, 3, 3]: the jitter (drawn from the generator when None).  Leaves the LAST frame posed.  -> rand."""
        F, res = len(self.frames), int(self.config.grid_resolution)
        if rand is None:
            rand = self._draw("uniform", F, res ** 3, 3, 3)
        occs, binaries, aabbs = [], [], []
        for idx in range(F):
            aabb = self.pose(self.corrected_params(idx))
            o, b = occ_grid.compute_test_occupancy_grid(self.occ_eval_fn(), aabb, res, 3, float(self.config.model["grid_prune_occ_thre"]), rand[idx])
            occs.append(o)
            binaries.append(b)
            aabbs.append(aabb)
        grid = self._new_grid(torch.stack(aabbs, 0).cpu(), F)
        grid.occs.copy_(torch.cat(occs, 0))
        grid.binaries.copy_(torch.cat(binaries, 0))
        self.grid = grid
        return rand

    def _point_at_level(self, t_idx: float) -> int:
        rs, lvl = self.rs, math.floor(t_idx * self.grid.levels)
        rs.binaries, rs.aabbs = self.grid.binaries[lvl:lvl + 1], self.grid.aabbs[lvl:lvl + 1]
        # the render step keys its cached forms of the grid by (address, version): another level may land at a known address
        rs._grid_bits = None
        rs._sort_grid_cache = None
        return lvl

    # ------------------------------------------------------------------ one step
    def draw_step(self, ph: Phase) -> Dict[str, Tensor]:
        """the step's random tensors, in the documented order"""
        cfg, n, F = self.config, self.n_rays, len(self.frames)
        m = cfg.model
        r = {}
        if self._perm is None or self._pos >= F:
            r["perm"] = self._draw("perm", F)
        r["words"] = self._draw("words", n)
        if m["background_color"] == "random":
            r["background"] = self._draw("uniform", 3)
        if m.get("randomized", True):
            r["jitter"] = self._draw("uniform", n)
        if ph.with_curvature:
            r["curv_u"] = self._draw("uniform", self.sample_cap, 3)
        if ph.enable_phys:
            spp = int(m["samples_per_pixel"])
            if ph.jitter_materials:
                r["material_jitter"] = self._draw("normal", self.sample_cap, 3)
            if m["render_mode"] == "uniform_light":
                r["light_u"] = self._draw("uniform", 512, 3)
                r["shuffle_u"] = self._draw("uniform", n, spp)
            else:
                r["light_u"] = self._draw("uniform", n * spp, 3)
        res = int(cfg.grid_resolution)
        if ph.grid_update:
            r["grid_rand"] = self._draw("uniform", res ** 3, 3)
        if ph.reinit_grid:
            r["reinit_rand"] = self._draw("uniform", F, res ** 3, 3, 3)
        return r

    def forward(self, ph: Phase, rays: Tensor, background: Tensor, r: Dict[str, Tensor]) -> Dict[str, Tensor]:
        """the model's output dict of the phase: forward_train_rf_ before phys_kick_in_step, forward_train_ from it"""
        m = self.config.model
        if not ph.enable_phys:
            return self.rs.forward_train_rf_(rays, r.get("jitter"), r.get("curv_u"), background)
        if m["render_mode"] == "light":
            self.emitter.update_pdf()                  # the light directions are drawn from the current lobes (:777-781)
        # a parametric emitter (EnvironmentLightSG) is shaded through the differentiable image of its current parameters
        env_base = self.emitter.generate_image() if hasattr(self.emitter, "generate_image") else None
        return self.rs.forward_train_(rays, self.material, self.emitter, int(m["samples_per_pixel"]), r["light_u"], jitter=r.get("jitter"),
                                      material_jitter=r.get("material_jitter"), background_color=background,
                                      global_illumination=bool(m["global_illumination"]), render_mode=m["render_mode"],
                                      shuffle_u=r.get("shuffle_u"), env_base=env_base, add_emitter=bool(m["add_emitter"]),
                                      curv_u=r.get("curv_u"))

    def loss(self, ph: Phase, out: Dict[str, Tensor], batch: Dict[str, Tensor]):
        """training_step's loss on the output dict -> (loss, {term: value}).  Before phys_kick_in_step the reference asks no module for
        its regularisers: the (zero) maps and the Lipschitz bound are left out."""
        lam = dict(ph.lam, sparsity_scale=float(self.config.loss.get("sparsity_scale", 1.0)))
        if not ph.enable_phys:
            out = {k: v for k, v in out.items() if not k.endswith("_loss_map")}
        wo = batch["rgb_wo_mask"] if self.config.model["add_emitter"] else None
        loss, terms = train_loss.fused_reference_loss(out, batch["rgb"], batch["alpha"], lam, self.material, wo)
        w = float(lam.get("lambda_lipshitz_bound", 0.0) or 0.0)
        if ph.enable_phys and w != 0.0:
            terms["lipshitz_bound"] = self.material.regularizations()["lipshitz_bound"]
            loss = loss + w * terms["lipshitz_bound"]
        return loss, terms

    def step(self) -> Dict:
        """one optimisation step; -> the step's record: `phase`, `frame`, `random` (the tensors drawn), `lr` (per parameter group, as
        used by this step), `pose_correction_enabled` (the frame was posed with its corrections), `loss`, `terms`, `num_samples`, `grid_level`, `grid_levels`, `out` (the model's output dict)."""
        cfg, frames, rs, F = self.config, self.frames, self.rs, len(self.frames)
        new_epoch = self._perm is None or self._pos >= F
        if new_epoch and self._perm is not None:
            self.epoch += 1
        ph = self.schedule.at(self.global_step, self.epoch)
        r = self.draw_step(ph)
        # 1. the frame: DataLoader(shuffle=True), one permutation per epoch
        if new_epoch:
            self._perm, self._pos = r["perm"].tolist(), 0
        idx = int(self._perm[self._pos])
        self._pos += 1
        # 2. / 3. the batch, composited over the step's background
        batch = dict(frames.batch(idx, words=r["words"]))
        bg_mode = cfg.model["background_color"]
        batch, background, _ = system.preprocess_data(batch, "train", background_color=bg_mode if bg_mode != "random" else "white",
                                                      background=r.get("background"))
        t_idx = idx / F                                        # the batch's t_idx, on the host
        # 4. pose: with the corrections of the frame's rows once the module's switch is on -- as the PREVIOUS step left it
        # (systems/base.py:109-111: the batch is preprocessed, i.e. posed, before update_step); tfs then carries the graph to them
        pc = self.pose_correction
        pc_on = pc is not None and pc.enable_pose_correction
        self.optimizer.zero_grad(set_to_none=True)
        params = self.corrected_params(idx, {k: batch[k] for k in ("betas", "body_pose", "global_orient", "transl")})
        self.pose(params)
        # 5. the modules' step counters (progressive hash levels, SH annealing, the pose-correction switch)
        for mod in (rs.geometry, rs.radiance, rs.density, pc):
            if mod is not None and hasattr(mod, "update_step"):
                mod.update_step(self.epoch, self.global_step)
        # 6. occupancy grid: EMA update of the frame's level, then (at its steps) one grid per frame
        if ph.grid_update:
            with torch.no_grad():
                self.grid.update_every_n_steps(self.global_step, t_idx, self.occ_eval_fn(), occ_thre=float(cfg.model["grid_prune_occ_thre"]),
                                               ema_decay=float(cfg.model["grid_prune_ema_decay"]), n=int(cfg.grid_update_every), rand=r["grid_rand"])
        if ph.reinit_grid:
            self.reinit_grids(r["reinit_rand"])
            self.pose(params)
        # 7. / 8.
        lvl = self._point_at_level(t_idx)
        rs.importance_sample = ph.importance_sample
        # 9. - 11.
        out = self.forward(ph, batch["rays"], background, r)
        n_samples = int(out["sdf_samples"].shape[0])
        if n_samples > self.sample_cap:
            raise RuntimeError(f"{n_samples} samples for {self.n_rays} rays: more than the {self.sample_cap} the random tensors were drawn for")
        for k in ("curv_u", "material_jitter"):
            if k in r:
                r[k] = r[k][:n_samples]
        loss, terms = self.loss(ph, out, batch)
        loss.backward()
        lr = [float(g["lr"]) for g in self.optimizer.param_groups]
        self.optimizer.step()
        if self.scheduler is not None:
            self.scheduler.step()
        rec = dict(global_step=self.global_step, epoch=self.epoch, phase=ph, frame=idx, random=r, lr=lr, loss=loss.detach(),
                   terms={k: v.detach() for k, v in terms.items()}, num_samples=out["num_samples"], grid_level=lvl,
                   grid_levels=int(self.grid.levels), background=background, batch=batch, out=out, pose_correction_enabled=bool(pc_on))
        self.global_step += 1
        return rec

    def fit(self, max_steps: Optional[int] = None, on_step: Optional[Callable[[Dict], None]] = None) -> Optional[Dict]:
        """steps until global_step reaches max_steps (default: trainer.max_steps); on_step(record) after every step (validation images,
        logging, checkpoints are the caller's: e.g. system.evaluate_frame every val_check_interval steps).  -> the last record."""
        max_steps = int(self.config.trainer["max_steps"]) if max_steps is None else int(max_steps)
        rec = None
        while self.global_step < max_steps:
            rec = self.step()
            if on_step is not None:
                on_step(rec)
        return rec

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self) -> Dict:
        """a copy of everything the next step depends on: the model under the reference's checkpoint keys (`model.geometry.*` ...,
        `model.occupancy_grid.*`, `model.emitter.*`), optimiser and scheduler state, the step / epoch counters with the epoch's
        permutation, and the generator's state."""
        sd = dict(checkpoint.reference_state_dict(self.rs, self.material))
        sd.update({"model.occupancy_grid." + k: v for k, v in self.grid.state_dict().items()})
        sd.update({"model.emitter." + k: v for k, v in self.emitter.state_dict().items()})
        if self.pose_correction is not None:
            sd.update({"model.pose_correction." + k: v for k, v in self.pose_correction.state_dict().items()})
            sd["pose_correction_enabled"] = bool(self.pose_correction.enable_pose_correction)
        sd["optimizer"] = self.optimizer.state_dict()
        sd["scheduler"] = self.scheduler.state_dict() if self.scheduler is not None else None
        sd["global_step"], sd["epoch"] = self.global_step, self.epoch
        sd["perm"], sd["pos"] = (list(self._perm) if self._perm is not None else None), self._pos
        sd["generator"] = self.generator.get_state()
        return copy.deepcopy(sd)

    def load_state_dict(self, sd: Dict) -> None:
        from . import fields
        model = {k: v for k, v in sd.items() if k.startswith("model.")}
        checkpoint.load_reference_state_dict(self.rs, model, self.material, strict=True)
        grid = {k[len("model.occupancy_grid."):]: v for k, v in model.items() if k.startswith("model.occupancy_grid.")}
        self.grid = self._new_grid(grid["aabbs"].cpu(), int(grid["binaries"].shape[0]))
        self.grid.load_state_dict(grid, strict=True)
        self.emitter.load_state_dict({k[len("model.emitter."):]: v for k, v in model.items() if k.startswith("model.emitter.")}, strict=True)
        if self.pose_correction is not None:
            self.pose_correction.load_state_dict({k[len("model.pose_correction."):]: v for k, v in model.items()
                                                  if k.startswith("model.pose_correction.")}, strict=True)
            self.pose_correction.enable_pose_correction = bool(sd.get("pose_correction_enabled", False))
        fields.params_changed()
        self.optimizer.load_state_dict(copy.deepcopy(sd["optimizer"]))
        if self.scheduler is not None and sd.get("scheduler") is not None:
            self.scheduler.load_state_dict(copy.deepcopy(sd["scheduler"]))
        self.global_step, self.epoch = int(sd["global_step"]), int(sd["epoch"])
        self._perm, self._pos = (list(sd["perm"]) if sd["perm"] is not None else None), int(sd["pos"])
        self.generator.set_state(sd["generator"])
