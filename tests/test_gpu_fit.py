"""GPU: fit.Trainer on the fixture recipe of tests/test_gpu_truth.py::test_evaluate_sequence (16 x 16 frames, the skeleton body, the
synthetic model with a 16 x 64 x 64 skinning grid, 32^3 occupancy grids), three frames, EdgeSampler with 64 rays, and the shipped
schedule compressed into eight steps:

    importance sampling from step 3 (kick-in 2, strict >), PBR from step 4, curvature until step 5, Lipschitz bound from step 5,
    grid update every 2 steps, one grid per frame from step 6, 3 warm-up steps of the learning rate.

Bounds: what two runs of the same forward compute is compared bit for bit (no forward kernel uses atomics); parameter gradients of two
routes to one step are held to 1e-3 of the tensor's largest entry, the project's bound for float atomics in the table backward
(tests/test_gpu_multiproc.py)."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
RES = 32
GRAD_BOUND = 1e-3


def config():
    from intrinsicavatar_amd import fit
    cfg = fit.FitConfig()
    cfg.model.update(importance_sample_kick_in_step=2, phys_kick_in_step=4, num_samples_per_ray=64)
    cfg.system.update(reinit_occupancy_grid_steps=[6], warmup_steps=3)
    cfg.loss.update(lambda_curvature=[1.5, 0.0, 5], lambda_lipshitz_bound=[5, 1.0e-5, 1.0e-5, 6], lambda_mask_mse=0.05, lambda_opaque=0.01,
                    lambda_sparsity=0.02)
    cfg.grid_update_every, cfg.grid_resolution, cfg.cano_pose = 2, RES, (0.0, 0.0, 0.0, 0.0)
    return cfg


def build(tmp, seed=5):
    from intrinsicavatar_amd import build as B, data, fields, fit, pbr, smpl, synthetic as S
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    B.build()
    GA = np.load(os.path.join(HERE, "golden", "golden_animation.npz"))
    np.savez(os.path.join(tmp, "cameras.npz"), intrinsic=np.eye(3), extrinsic=np.eye(4), height=np.int64(1080), width=np.int64(1080))
    np.savez(os.path.join(tmp, "poses.npz"), poses=GA["aist_in_poses"], trans=GA["aist_in_trans"])
    host = data.animation_host(tmp, np.zeros(10), start=0, end=8, skip=4, downscale=67.5)
    assert (host["height"], host["width"]) == (16, 16) and len(host["transl"]) == 3
    rng = np.random.default_rng(3)
    y, x = np.mgrid[0:16, 0:16]
    body_mask = (((x - 7.5) / 4.6) ** 2 + ((y - 8) / 6.6) ** 2 <= 1).astype(np.float32)
    masks = np.stack([body_mask, np.roll(body_mask, 1, axis=1), np.roll(body_mask, -1, axis=1)])
    images = torch.from_numpy(rng.integers(0, 256, (3, 16, 16, 3), dtype=np.uint8)).to(DEV)
    frames = data.TrainingFrames(images, torch.from_numpy(masks).to(DEV), host["K"], np.linalg.inv(host["w2c"][0]),
                                 {k: host[k] for k in ("betas", "body_pose", "global_orient", "transl")},
                                 sampler=data.EdgeSampler(64, kernel_size=5), near=host["near"], far=host["far"])
    rs, _, _ = S.build_frame(DEV, 16, 16, pose_seed=0, beta=0.01, num_samples_per_ray=64, grid_D=16, grid_H=64, grid_W=64, smooth_iters=5,
                             hash_amp=2e-3)
    mat = fields.VolumeMaterial(seed=2).to(DEV)
    env = pbr.EnvironmentLightSG(num_SGs=8, base_res=16, seed=1).to(DEV)
    eye = torch.eye(24, device=DEV)
    body = smpl.SMPLKinematics(torch.from_numpy(S.JOINTS).to(DEV), torch.zeros((24, 3, 10), device=DEV), torch.zeros((207, 72), device=DEV),
                               eye, S.PARENTS.tolist(), eye)
    return fit.Trainer(rs, mat, env, frames, body, config(), torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """two identically seeded trainers and their initial state; every test starts from that state"""
    a, b = build(str(tmp_path_factory.mktemp("fit_a"))), build(str(tmp_path_factory.mktemp("fit_b")))
    return a, b, a.state_dict()


def params_of(tr):
    return [p for g in tr.optimizer.param_groups for p in g["params"]]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


def test_eight_steps_follow_the_schedule(pair):
    from intrinsicavatar_amd import optim
    tr, _, sd0 = pair
    tr.load_state_dict(sd0)
    start = [p.detach().clone() for p in params_of(tr)]
    ref_opt, ref_sched = optim.reference_optimizer(tr.rs, material=tr.material, emitter=tr.emitter, warmup_steps=3)
    rf_terms = {"rgb_mse", "rgb_l1", "eikonal", "mask_mse", "mask_bce", "opaque", "sparsity", "curvature"}
    pbr_terms = rf_terms | {"rgb_phys_mse", "rgb_phys_l1", "rgb_demodulated", "normal_orientation", "albedo_smoothness", "roughness_smoothness",
                            "metallic_smoothness"}
    for s in range(8):
        before = tr.grid.binaries.clone()
        rec = tr.step()
        ph, out = rec["phase"], rec["out"]
        assert rec["global_step"] == s and tr.global_step == s + 1
        assert (ph.enable_phys, ph.importance_sample, ph.with_curvature, ph.grid_update, ph.reinit_grid) == \
            (s >= 4, s > 2, s < 5, s % 2 == 0, s == 6), s
        assert tr.rs.importance_sample == (s > 2)
        # the phase's output dict
        assert ("comp_rgb_phys_full" in out) == ("comp_albedo_full" in out) == ("rays_valid_phys_bg" in out and s >= 4), s
        assert {"comp_rgb_full", "rays_valid_full", "rays_valid_phys_full", "sdf_samples", "sdf_grad_samples", "sdf_laplace_samples", "opacity",
                "comp_rgb_bg", "num_samples_full", "albedo_smoothness_loss_map", "depth", "comp_normal"} <= set(out), s
        if s < 4:
            assert not bool(out["rays_valid_phys_full"].any()) and not bool(out["albedo_smoothness_loss_map"].any())
        else:
            assert bool(out["rays_valid_phys_full"].any())
        # the loss terms
        want = (pbr_terms if s >= 4 else rf_terms) | ({"lipshitz_bound"} if s >= 5 else set())
        assert set(rec["terms"]) == want, (s, sorted(set(rec["terms"]) ^ want))
        assert all(math.isfinite(float(v)) for v in rec["terms"].values()) and math.isfinite(float(rec["loss"])), (s, rec["terms"])
        # curvature reaches the dict while its weight is on -- on the PBR path too (step 4)
        lap = float(out["sdf_laplace_samples"].detach().abs().max())
        assert (lap > 0.0) == (s < 5), (s, lap)
        assert (float(rec["terms"]["curvature"]) > 0.0) == (s < 5)
        # learning rate
        assert rec["lr"] == [float(g["lr"]) for g in ref_opt.param_groups], s
        ref_sched.step()
        # grids
        assert rec["grid_levels"] == (1 if s < 6 else 3) and tuple(tr.grid.binaries.shape) == (rec["grid_levels"], RES, RES, RES)
        assert tr.rs.binaries.data_ptr() == tr.grid.binaries[rec["grid_level"]].data_ptr()
        if s != 6:
            after = tr.grid.binaries
            for lvl in range(after.shape[0]):
                if not (s % 2 == 0 and lvl == rec["grid_level"]):
                    assert torch.equal(before[lvl], after[lvl]), (s, lvl)
        assert bool(tr.grid.binaries[rec["grid_level"]].any())
    moved = [not torch.equal(p0, p.detach()) for p0, p in zip(start, params_of(tr))]
    assert all(moved), moved


def replay_by_hand(tr, rec):
    """the calls of one step, written out, with the record's random tensors; no optimiser step.  -> (loss, terms, out)"""
    from intrinsicavatar_amd import render, smpl, system, train_loss
    rs, cfg, r, ph = tr.rs, tr.config, rec["random"], rec["phase"]
    idx, F, step = rec["frame"], len(tr.frames), rec["global_step"]
    batch = dict(tr.frames.batch(idx, words=r["words"]))
    batch, bg, _ = system.preprocess_data(batch, "train", background=r["background"])
    out = tr.body.forward(batch["betas"], batch["body_pose"], batch["global_orient"], batch["transl"])
    tfs, w2s = smpl.deformer_transforms(out["A"], tr.A_rest_inv)
    rs.deformer.prepare(tfs, w2s[0])
    rs.geometry.prepare_bbox(rs.deformer.bbox)
    rs.radiance.prepare_bbox(rs.deformer.bbox)
    rs.geometry.update_step(0, step)
    rs.radiance.update_step(0, step)
    beta_t = rs.density.get_beta().detach().reshape(1)
    occ_eval_fn = lambda x: render.laplace_alpha(rs.deformer.deform(x, rs.geometry)["sdf"], rs.render_step_size, beta_t)      # noqa: E731
    if ph.grid_update:
        tr.grid.update_every_n_steps(step, idx / F, occ_eval_fn, occ_thre=0.001, ema_decay=0.8, n=2, rand=r["grid_rand"])
    lvl = math.floor(idx / F * tr.grid.levels)
    rs.binaries, rs.aabbs = tr.grid.binaries[lvl:lvl + 1], tr.grid.aabbs[lvl:lvl + 1]
    rs._grid_bits = rs._sort_grid_cache = None
    rs.importance_sample = ph.importance_sample
    for p in params_of(tr):
        p.grad = None
    lam = dict(ph.lam, sparsity_scale=1.0)
    if not ph.enable_phys:
        d = rs.forward_train_rf_(batch["rays"], r["jitter"], r["curv_u"], bg)
        loss, terms = train_loss.fused_reference_loss({k: v for k, v in d.items() if not k.endswith("_loss_map")}, batch["rgb"], batch["alpha"],
                                                      lam, tr.material)
    else:
        d = rs.forward_train_(batch["rays"], tr.material, tr.emitter, 512, r["light_u"], jitter=r["jitter"], material_jitter=r["material_jitter"],
                              background_color=bg, global_illumination=True, render_mode="uniform_light", shuffle_u=r["shuffle_u"],
                              env_base=tr.emitter.generate_image(), curv_u=r["curv_u"])
        loss, terms = train_loss.fused_reference_loss(d, batch["rgb"], batch["alpha"], lam, tr.material)
        if lam["lambda_lipshitz_bound"]:
            loss = loss + lam["lambda_lipshitz_bound"] * tr.material.regularizations()["lipshitz_bound"]
    loss.backward()
    return loss.detach(), terms, d


@pytest.mark.parametrize("first_step", [0, 4])
def test_a_step_is_what_its_record_says(pair, first_step):
    """step 0 (radiance field) and step 4 (the first PBR step, curvature still on): Trainer.step() on one model, the same calls by hand
    with the record's random tensors on an identically seeded second one"""
    a, b, sd0 = pair
    sd = dict(sd0, global_step=first_step)
    a.load_state_dict(sd)
    b.load_state_dict(sd)
    rec = a.step()
    assert rec["global_step"] == first_step and rec["phase"].enable_phys == (first_step == 4) and rec["phase"].with_curvature
    grads_a = [p.grad.clone() if p.grad is not None else None for p in params_of(a)]
    loss, terms, out = replay_by_hand(b, rec)
    assert same_bits(loss, rec["loss"]) and same_bits(out["num_samples"], rec["num_samples"])
    for k, v in rec["terms"].items():
        if k != "lipshitz_bound":
            assert same_bits(terms[k], v), k
    assert same_bits(out["comp_rgb_full"], rec["out"]["comp_rgb_full"])
    n_grads = 0
    for ga, pb in zip(grads_a, params_of(b)):
        assert (ga is None) == (pb.grad is None)
        if ga is not None:
            top = float(ga.abs().max())
            err = float((ga - pb.grad).abs().max())
            print(f"step {first_step} gradient {tuple(ga.shape)}: max difference {err:.3e}, largest entry {top:.3e}")
            assert err <= GRAD_BOUND * top, (tuple(ga.shape), err, top)
            n_grads += top > 0.0
    assert n_grads >= (10 if first_step == 4 else 6)


def test_state_dict_round_trip(pair):
    from intrinsicavatar_amd import checkpoint
    a, b, sd0 = pair
    a.load_state_dict(sd0)
    b.load_state_dict(sd0)
    for _ in range(3):
        a.step()
    sd = a.state_dict()
    b.load_state_dict(sd)
    assert b.global_step == a.global_step == 3 and b.epoch == a.epoch and b._perm == a._perm and b._pos == a._pos
    n_state = 0
    for pa, pb in zip(params_of(a), params_of(b)):
        assert same_bits(pa.detach(), pb.detach())
        sa, sb = a.optimizer.state.get(pa, {}), b.optimizer.state.get(pb, {})
        assert set(sa) == set(sb)                          # (material and emitter have no state yet: three radiance-field steps)
        if sa:
            n_state += 1
            assert float(sa["step"]) == float(sb["step"]) == 3.0
            assert same_bits(sa["exp_avg"], sb["exp_avg"]) and same_bits(sa["exp_avg_sq"], sb["exp_avg_sq"])
    assert n_state >= 15
    for k in ("resolution", "aabbs", "occs", "binaries"):
        assert same_bits(getattr(a.grid, k), getattr(b.grid, k)), k
    assert [g["lr"] for g in a.optimizer.param_groups] == [g["lr"] for g in b.optimizer.param_groups]
    # the model keys are the reference's: they load into the components with strict=True
    model = {k: v for k, v in sd.items() if k.startswith("model.")}
    assert any(k.startswith("model.occupancy_grid.") for k in model) and any(k.startswith("model.emitter.") for k in model)
    rest = checkpoint.load_reference_state_dict(b.rs, model, b.material, strict=True)
    assert set(rest) == {"emitter"}
    ra, rb = a.step(), b.step()
    assert ra["frame"] == rb["frame"] and ra["lr"] == rb["lr"] and set(ra["random"]) == set(rb["random"])
    for k, v in ra["random"].items():
        assert same_bits(v, rb["random"][k]), k
    assert same_bits(ra["num_samples"], rb["num_samples"])


def test_reinit_grids_is_the_per_frame_test_grid(pair):
    from intrinsicavatar_amd import occ_grid
    tr, _, sd0 = pair
    tr.load_state_dict(sd0)
    rand = tr.reinit_grids()
    assert tuple(rand.shape) == (3, RES ** 3, 3, 3) and tr.grid.levels == 3 and tr.grid.training
    for idx in range(3):
        aabb = tr.pose(tr._frame_params(idx))
        occs, binaries = occ_grid.compute_test_occupancy_grid(tr.occ_eval_fn(), aabb, RES, 3, 0.001, rand[idx])
        assert same_bits(tr.grid.aabbs[idx], aabb)
        assert same_bits(tr.grid.occs[idx * RES ** 3:(idx + 1) * RES ** 3], occs)
        assert same_bits(tr.grid.binaries[idx], binaries[0]) and bool(binaries.any()) and not bool(binaries.all())
    assert not same_bits(tr.grid.aabbs[0], tr.grid.aabbs[1])


@pytest.mark.parametrize("change", [
    dict(enable_pose_correction=True), dict(optimize_betas=True), dict(reinit_optimizer_steps=[5000]), dict(world_size=2),
    dict(system=dict(reinit_shape_every_n_steps=2000)), dict(system=dict(pbr_loss_only=True)), dict(loss=dict(lambda_distortion=0.01)),
    dict(loss=dict(lambda_albedo=1.0)), dict(model=dict(learned_background=True))])
def test_out_of_scope_options_raise(change):
    """the Trainer refuses them before it touches anything else"""
    from intrinsicavatar_amd import fit
    cfg = config()
    for k, v in change.items():
        getattr(cfg, k).update(v) if isinstance(v, dict) else setattr(cfg, k, v)
    with pytest.raises(NotImplementedError, match="out of scope"):
        fit.Trainer(None, None, None, None, None, cfg)
