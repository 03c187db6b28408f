"""GPU: fit.Trainer with a pose_correction.PoseCorrection module, on the fixture recipe of tests/test_gpu_fit.py (its `config` and
`build`, copied) with enable_pose_correction, pose_correction_start_step = 1 and PBR from step 4:

    steps 0 - 2  the switch is off while the frame is posed (it turns on DURING step 2, after the pose): the step of a trainer
                 without the module
    step 3       the first step that adds corrections (start step + 2), radiance-field dict
    steps 4 - 7  corrections through the PBR dict; step 6 re-initialises the grids with every frame's corrected parameters

One run of eight steps (and three of the trainer without the module) is shared by the tests; tests that step further start from the
state after those eight.

What "the step of a trainer without the module" can mean: two identically seeded trainers WITHOUT the module do not keep bit-identical
parameters -- the weight-gradient kernels of the two MLP heads and the split buckets of the hash-table backward add in float atomics
(DESIGN 4.4), and Adam (eps 1e-15) turns a last-bit difference of a gradient into a last-bit difference of the parameter.  Measured
on the MI355X, module-less trainer against module-less trainer, after ONE step: up to 261 of 2240 gradient words of a geometry weight
matrix differ (by <= 1.5e-8 of entries up to 0.18), 10 of 64 words of its bias differ afterwards; after three steps 275 of 12.6 M
hash-table words.  The same figures separate the trainer with the module from the one without.  So the comparison is made per step
from the SAME state (the second trainer takes the first one's parameters and Adam moments before each step): everything the forward
pass produces -- random draws, loss, every loss term, sample count, the image -- must have the same bits; the parameters after the
step must agree within the a-priori bound of two Adam steps that saw different roundings of one gradient, 2 x the group's learning rate
(an Adam update is at most lr x (1 - beta1) / sqrt(1 - beta2) = lr for betas (0.9, 0.99), in either direction)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
RES = 32
NAMES = ("pose_correction", "shape_correction", "global_orient_correction", "transl_correction")


def config(pose_correction):
    from intrinsicavatar_amd import fit
    cfg = fit.FitConfig()
    cfg.model.update(importance_sample_kick_in_step=2, phys_kick_in_step=4, num_samples_per_ray=64)
    cfg.system.update(reinit_occupancy_grid_steps=[6], warmup_steps=3)
    cfg.loss.update(lambda_curvature=[1.5, 0.0, 5], lambda_lipshitz_bound=[5, 1.0e-5, 1.0e-5, 6], lambda_mask_mse=0.05, lambda_opaque=0.01,
                    lambda_sparsity=0.02)
    cfg.grid_update_every, cfg.grid_resolution, cfg.cano_pose = 2, RES, (0.0, 0.0, 0.0, 0.0)
    if pose_correction:
        cfg.enable_pose_correction, cfg.pose_correction_start_step = True, 1
    return cfg


def build(tmp, pose_correction, seed=5):
    from intrinsicavatar_amd import build as B, data, fields, fit, pbr, smpl, synthetic as S
    from intrinsicavatar_amd.pose_correction import PoseCorrection
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
    pc = PoseCorrection(len(frames), enable_pose_correction=True, pose_correction_start_step=1) if pose_correction else None
    return fit.Trainer(rs, mat, env, frames, body, config(pose_correction), torch.Generator().manual_seed(seed), pose_correction=pc)


def params_of(tr, name=None):
    return [p for g in tr.optimizer.param_groups for p in g["params"] if name is None or g["name"] == name]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


def weights(tr):
    return {n: getattr(tr.pose_correction, n).weight.detach().clone() for n in NAMES}


def take_state(b, a):
    """b (no module) takes a's parameters and Adam moments, in place; the step counters, the generators and the grids already agree"""
    from intrinsicavatar_amd import fields
    with torch.no_grad():
        for pa, pb in zip(params_of(a), params_of(b)):
            pb.copy_(pa)
            sa, sb = a.optimizer.state.get(pa, {}), b.optimizer.state.get(pb, {})
            assert set(sa) == set(sb)
            for k in ("exp_avg", "exp_avg_sq"):
                if k in sa:
                    sb[k].copy_(sa[k])
    fields.params_changed()


def light(rec):
    """a step's record without the output dict and the batch (the run keeps eight of them)"""
    return {k: v for k, v in rec.items() if k not in ("out", "batch")}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """a: the trainer with the module, stepped eight times; b: the same without it, stepped three times, each from a's state;
    c: a's twin, untouched.  per step of a: record, the module's weights before / after, its gradients, the tfs the step was posed
    with and tfs.grad."""
    a, b, c = (build(str(tmp_path_factory.mktemp("pc_" + n)), n != "b") for n in "abc")
    dfm = a.rs.deformer
    held = {}
    prepare = dfm.prepare

    def keeping(tfs, w2s):
        prepare(tfs, w2s)
        held["tfs"] = dfm.tfs
        if dfm.tfs.requires_grad:
            dfm.tfs.retain_grad()

    dfm.prepare = keeping
    steps, plain = [], []
    for s in range(8):
        if s < 3:
            take_state(b, a)
            rb = b.step()
            plain.append(dict(rec=light(rb), image=rb["out"]["comp_rgb_full"].detach().clone(), params=[p.detach().clone() for p in params_of(b)]))
        before = weights(a)
        rec = a.step()
        pc = a.pose_correction
        steps.append(dict(rec=light(rec), before=before, after=weights(a), batch={k: rec["batch"][k].detach().clone() for k in
                                                                                   ("betas", "body_pose", "global_orient", "transl")},
                          grad={n: (getattr(pc, n).weight.grad.detach().clone() if getattr(pc, n).weight.grad is not None else None) for n in NAMES},
                          tfs_requires_grad=bool(held["tfs"].requires_grad),
                          tfs_grad=held["tfs"].grad.detach().clone() if held["tfs"].requires_grad and held["tfs"].grad is not None else None,
                          enable_phys=rec["phase"].enable_phys, image=rec["out"]["comp_rgb_full"].detach().clone() if s < 3 else None,
                          params=[p.detach().clone() for p in params_of(a)] if s < 3 else None))
    dfm.prepare = prepare
    return dict(a=a, b=b, c=c, steps=steps, plain=plain, sd8=a.state_dict())


def test_constructor_takes_the_flag_only_with_a_module(run):
    from intrinsicavatar_amd import fit
    a = run["a"]
    assert a.config.enable_pose_correction and a.pose_correction is not None
    assert all(p.is_cuda for p in a.pose_correction.parameters())
    with pytest.raises(NotImplementedError, match="out of scope"):
        fit.Trainer(a.rs, a.material, a.emitter, a.frames, a.body, config(True), torch.Generator().manual_seed(0))
    assert run["b"].pose_correction is None


def test_first_three_steps_are_the_trainer_without_the_module(run):
    for s in range(3):
        st, pl = run["steps"][s], run["plain"][s]
        ra, rb = st["rec"], pl["rec"]
        assert not ra["pose_correction_enabled"] and not rb["pose_correction_enabled"] and not st["tfs_requires_grad"]
        assert ra["frame"] == rb["frame"] and same_bits(ra["loss"], rb["loss"]) and same_bits(ra["num_samples"], rb["num_samples"])
        assert set(ra["random"]) == set(rb["random"]) and set(ra["terms"]) == set(rb["terms"])
        for k, v in ra["random"].items():
            assert same_bits(v, rb["random"][k]), (s, k)
        for k, v in ra["terms"].items():
            assert same_bits(v, rb["terms"][k]), (s, k)
        assert same_bits(st["image"], pl["image"]), s
        assert ra["lr"][:-1] == rb["lr"] and len(ra["lr"]) == len(rb["lr"]) + 1
        n = len(pl["params"])
        assert len(st["params"]) == n + 4
        lrs = [lr for g, lr in zip(run["b"].optimizer.param_groups, rb["lr"]) for _ in g["params"]]
        n_diff = 0
        for pa, pb, lr in zip(st["params"][:n], pl["params"], lrs):
            assert float((pa - pb).abs().max()) <= 2.0 * lr, (s, tuple(pa.shape), float((pa - pb).abs().max()), lr)
            n_diff += int((pa.view(torch.int32) != pb.view(torch.int32)).sum())
        print(f"step {s}: {n_diff} of {sum(p.numel() for p in pl['params'])} parameter words differ from the trainer without the module")
        assert all(float(w.abs().max()) == 0.0 for w in st["after"].values()), s
        assert all(g is None for g in st["grad"].values()), s


def test_corrections_start_at_step_three_and_move_the_visited_rows(run):
    steps = run["steps"]
    assert [st["rec"]["pose_correction_enabled"] for st in steps] == [False] * 3 + [True] * 5           # start step 1: first at 1 + 2
    assert [st["tfs_requires_grad"] for st in steps] == [False] * 3 + [True] * 5
    assert [st["enable_phys"] for st in steps] == [False] * 4 + [True] * 4
    visited = set()
    for s in range(3, 8):
        st = steps[s]
        i = st["rec"]["frame"]
        visited.add(i)
        before, after = st["before"]["pose_correction"], st["after"]["pose_correction"]
        g = st["grad"]["pose_correction"]
        assert g is not None and g.shape == (3, 69) and bool(torch.isfinite(g).all())
        assert float(g[i].abs().max()) > 0.0, s                                    # radiance-field dict (3) and PBR dict (4 ..) alike
        assert all(float(g[j].abs().max()) == 0.0 for j in range(3) if j != i), s
        assert not torch.equal(before[i], after[i]), s
        for j in range(3):
            if j not in visited:                                                   # no gradient yet, nothing to decay
                assert float(after[j].abs().max()) == 0.0, (s, j)
        # the shape row is carried, never added, never trained
        assert st["grad"]["shape_correction"] is None and float(st["after"]["shape_correction"].abs().max()) == 0.0
        for n in ("global_orient_correction", "transl_correction"):
            assert st["grad"][n] is not None and bool(torch.isfinite(st["grad"][n]).all())
    assert visited == {0, 1, 2}


def test_gradient_is_the_kinematic_one(run):
    """step 3: pose_correction.weight.grad[i] = d loss / d body_pose, by fp64 CPU autograd of smpl + deformer_transforms fed with the
    step's tfs.grad.  rtol 1e-4 per entry; atol 256 x 2^-24 of the largest entry: an entry is a sum over the 24 x 12 entries of tfs
    of products that a kinematic chain of up to ~10 joints produced in the device's arithmetic, and a small entry is the difference
    of large ones."""
    from intrinsicavatar_amd import smpl, synthetic as S
    a, st = run["a"], run["steps"][3]
    i = st["rec"]["frame"]
    assert st["tfs_grad"] is not None and float(st["tfs_grad"].abs().max()) > 0
    D = lambda t: t.detach().cpu().double()      # noqa: E731
    eye = torch.eye(24, dtype=torch.float64)
    body = smpl.SMPLKinematics(torch.from_numpy(S.JOINTS).double(), torch.zeros((24, 3, 10), dtype=torch.float64),
                               torch.zeros((207, 72), dtype=torch.float64), eye, S.PARENTS.tolist(), eye)
    b = st["batch"]
    pose = (D(b["body_pose"]) + D(st["before"]["pose_correction"][i:i + 1])).requires_grad_(True)
    orient = (D(b["global_orient"]) + D(st["before"]["global_orient_correction"][i:i + 1])).requires_grad_(True)
    transl = (D(b["transl"]) + D(st["before"]["transl_correction"][i:i + 1])).requires_grad_(True)
    out = body.forward(D(b["betas"]), pose, orient, transl)
    tfs, _ = smpl.deformer_transforms(out["A"], D(a.A_rest_inv), dtype=torch.float64)
    (tfs * D(st["tfs_grad"])).sum().backward()
    want = pose.grad[0]
    got = D(st["grad"]["pose_correction"][i])
    top = float(want.abs().max())
    err = (got - want).abs()
    print(f"d loss / d body_pose: max abs difference {float(err.max()):.3e}, largest entry {top:.3e}, "
          f"worst relative {float((err / want.abs().clamp_min(1e-300)).max()):.3e}")
    assert top > 0
    assert bool((err <= 1e-4 * want.abs() + 256 * 2.0 ** -24 * top).all())
    # the deformer works in the SMPL-root frame (tfs = inverse(A_root) A): the root rotation and the translation cancel, their rows
    # receive rounding-level gradient only
    for n, ref in (("global_orient_correction", orient), ("transl_correction", transl)):
        gn = float(st["grad"][n][i].abs().max())
        g64 = float(ref.grad.abs().max()) if ref.grad is not None else 0.0
        print(f"{n}: largest gradient entry {gn:.3e} (fp64: {g64:.3e})")
        assert gn < 1e-3 * top and g64 < 1e-9 * top


def test_optimizer_group(run):
    from intrinsicavatar_amd import optim
    a, b = run["a"], run["b"]
    groups = a.optimizer.param_groups
    assert [g["name"] for g in groups] == [g["name"] for g in b.optimizer.param_groups] + ["pose_correction"]
    pc = groups[-1]
    assert pc["weight_decay"] == 1e-5 and pc["initial_lr"] == 1e-4 and len(pc["params"]) == 4
    assert {id(p) for p in pc["params"]} == {id(p) for p in a.pose_correction.parameters()}
    for ga, gb in zip(groups, b.optimizer.param_groups):
        assert (ga["initial_lr"], ga["weight_decay"], ga["betas"], ga["eps"]) == (gb["initial_lr"], gb["weight_decay"], gb["betas"], gb["eps"])
    ref_opt, ref_sched = optim.reference_optimizer(a.rs, material=a.material, emitter=a.emitter, warmup_steps=3, pose_correction=a.pose_correction)
    plain_opt, plain_sched = optim.reference_optimizer(a.rs, material=a.material, emitter=a.emitter, warmup_steps=3)
    for s, st in enumerate(run["steps"]):
        lr = st["rec"]["lr"]
        assert lr == [float(g["lr"]) for g in ref_opt.param_groups], s
        assert lr[:-1] == [float(g["lr"]) for g in plain_opt.param_groups], s                # the other groups: exactly today's
        factor = lr[0] / 1e-3
        assert abs(lr[-1] - 1e-4 * factor) <= 1e-12 * lr[-1], (s, lr[-1], factor)
        ref_sched.step()
        plain_sched.step()


def test_reinit_grids_poses_every_frame_with_its_corrections(run):
    from intrinsicavatar_amd import occ_grid
    a = run["a"]
    a.load_state_dict(run["sd8"])
    assert a.pose_correction.enable_pose_correction
    with torch.no_grad():
        for n in NAMES:
            getattr(a.pose_correction, n).weight.zero_()
        a.pose_correction.pose_correction.weight[1, 45:51] = 0.4               # joints 16 / 17: the upper arms
    rand = a.reinit_grids()
    assert a.grid.levels == 3
    for idx in range(3):
        with torch.no_grad():
            plain = a.pose(a._frame_params(idx))
            aabb = a.pose(a.corrected_params(idx))
        occs, binaries = occ_grid.compute_test_occupancy_grid(a.occ_eval_fn(), aabb, RES, 3, 0.001, rand[idx])
        assert same_bits(a.grid.aabbs[idx], aabb), idx
        assert same_bits(a.grid.occs[idx * RES ** 3:(idx + 1) * RES ** 3], occs) and same_bits(a.grid.binaries[idx], binaries[0])
        assert same_bits(plain, aabb) == (idx != 1), idx


def test_state_dict_round_trip(run):
    from intrinsicavatar_amd import checkpoint
    a, c, sd = run["a"], run["c"], run["sd8"]
    keys = {f"model.pose_correction.{n}.weight" for n in NAMES}
    assert keys <= set(sd) and {k for k in sd if k.startswith("model.pose_correction.")} == keys
    assert float(sd["model.pose_correction.pose_correction.weight"].abs().max()) > 0
    a.load_state_dict(sd)
    c.load_state_dict(sd)
    assert c.global_step == a.global_step == 8 and c.pose_correction.enable_pose_correction
    for n in NAMES:
        assert same_bits(getattr(a.pose_correction, n).weight.detach(), getattr(c.pose_correction, n).weight.detach())
    for pa, pc in zip(params_of(a, "pose_correction"), params_of(c, "pose_correction")):
        sa, sc = a.optimizer.state.get(pa, {}), c.optimizer.state.get(pc, {})
        assert set(sa) == set(sc)
        if sa:
            assert float(sa["step"]) == float(sc["step"]) == 5.0 and same_bits(sa["exp_avg"], sc["exp_avg"])
    # the test-mode loader of a reference checkpoint drops the module's keys
    model = {k: v for k, v in sd.items() if k.startswith("model.")}
    rest = checkpoint.load_reference_state_dict(c.rs, model, c.material, strict=True)
    assert set(rest) == {"emitter"}
    assert not any("pose_correction" in k for part in checkpoint.split_reference_state_dict(model).values() for k in part)
    ra, rc = a.step(), c.step()
    assert ra["pose_correction_enabled"] and rc["pose_correction_enabled"] and ra["frame"] == rc["frame"] and ra["lr"] == rc["lr"]
    assert same_bits(ra["loss"], rc["loss"]) and same_bits(ra["num_samples"], rc["num_samples"])
    for k, v in ra["random"].items():
        assert same_bits(v, rc["random"][k]), k
    assert same_bits(ra["out"]["comp_rgb_full"], rc["out"]["comp_rgb_full"])
    for n in NAMES:
        wa, wc = getattr(a.pose_correction, n).weight, getattr(c.pose_correction, n).weight
        assert same_bits(wa.detach(), wc.detach()), n
        assert (wa.grad is None) == (wc.grad is None) and (wa.grad is None or same_bits(wa.grad, wc.grad)), n
