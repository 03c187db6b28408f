#!/usr/bin/env python3
"""What the fused training loss saves on the launch-bound 4096-ray step, and what a whole fit.Trainer step costs, on the scene of
tools/config4_bench.py (uniform_light, spp 512), all in ONE process:

    1  forward_backward_phys(loss_config=lam)   train_phys.reference_training_loss in torch: the route before the fused loss
    2  the same output dict, train_loss.fused_reference_loss
    3  fit.Trainer.step()                        batch, pose, grid (one EMA update per 20 steps), forward, fused loss, backward, Adam

Cases 1 and 2 share rays, targets, random tensors and loss weights (the shipped schedule at step 13 000: PBR on, curvature off, so that
both routes compute the same terms).  Every case gets 10 warm-up steps; then the cases take turns, `--repeat` timings of `--steps` steps
each; launches and read-backs of one step from tools/launch_audit.py.    python tools/fit_step_bench.py [--out profiles/fit_step.json]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

POSE = "male-3-casual:0"


def timed(cases, steps, repeat):
    """{name: [ms per step, ...]}: every case warmed up, then the cases take turns `repeat` times (drift of the shared host and of the
    clocks lands on all of them alike)"""
    for _, step in cases:
        for _ in range(10):
            step()
    runs = {name: [] for name, _ in cases}
    for _ in range(repeat):
        for name, step in cases:
            step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            runs[name].append(round((time.perf_counter() - t0) / steps * 1e3, 3))
    return runs


def trainer_on_bench_scene(rs, rays, mat, sg, dev, hw, n_batch):
    """a fit.Trainer whose one frame is the bench frame: the skeleton body in the pose of the synthetic rig, the mask of the rendered
    subject, a random image"""
    from intrinsicavatar_amd import data, fit, smpl, synthetic as S
    pose72, transl = S.parse_pose(POSE)
    with torch.no_grad():
        mask = (rs.forward(rays)["opacity"][:, 0] > 0.5).float().reshape(1, hw, hw)
    g = torch.Generator().manual_seed(11)
    images = torch.randint(0, 256, (1, hw, hw, 3), generator=g, dtype=torch.uint8).to(dev)
    K = S.K_1080.copy()
    K[:2] /= 1080.0 / hw
    params = dict(betas=np.zeros(10), body_pose=np.asarray(pose72[3:])[None], global_orient=np.asarray(pose72[:3])[None],
                  transl=np.asarray(transl)[None])
    frames = data.TrainingFrames(images, mask, K, np.eye(4), params, sampler=data.EdgeSampler(n_batch))
    eye = torch.eye(24, device=dev)
    body = smpl.SMPLKinematics(torch.from_numpy(S.JOINTS).to(dev), torch.zeros((24, 3, 10), device=dev), torch.zeros((207, 72), device=dev),
                               eye, S.PARENTS.tolist(), eye)
    cfg = fit.FitConfig()
    cfg.cano_pose = (0.0, 0.0, 0.0, 0.0)
    tr = fit.Trainer(rs, mat, sg, frames, body, cfg, torch.Generator(device=dev).manual_seed(5))
    tr.global_step = 13000          # PBR phase, curvature off; a grid-update step, so the first step fills the one-level grid
    return tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--n-batch", type=int, default=4096)
    ap.add_argument("--hw", type=int, default=540)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_step.json"))
    args = ap.parse_args()
    import bench as B
    import launch_audit
    from intrinsicavatar_amd import build, fit, optim, pbr, train_loss
    build.build()
    dev = "cuda:0"
    torch.cuda.memory._set_allocator_settings("roundup_power2_divisions:8")
    rs, rays, _, mat, sg = B.build_headline(dev, args.hw, 1024, 0, POSE)
    bg = torch.ones(3, device=dev)
    n, spp = args.n_batch, 512
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        hit = torch.nonzero(rs.forward(rays)["opacity"][:, 0] > 0.5)[:, 0]
    batch = rays[hit[torch.randint(0, hit.shape[0], (n,), generator=g).to(dev)]].contiguous()
    target, tmask = torch.rand((n, 3), generator=g).to(dev), torch.ones(n, device=dev)
    light_u, shuffle_u = torch.rand((spp, 3), generator=g).to(dev), torch.rand((n, spp), generator=g).to(dev)
    mj = torch.randn((n * 168, 3), generator=g).to(dev)
    lam = dict(fit.Schedule().at(13000).lam, sparsity_scale=1.0)
    params = rs.parameters() + [p for p in mat.parameters() if p.requires_grad] + list(sg.parameters())
    opt, sched = optim.reference_optimizer(rs, material=mat, emitter=sg)

    def dict_step(fused):
        def step():
            for p in params:
                p.grad = None
            img = sg.generate_image()
            leaf = img.detach().requires_grad_(True)
            emitter = pbr.EnvironmentLightTensor(leaf.detach())
            emitter.update_pdf()
            kw = dict(render_mode="uniform_light", env_base=leaf, background_color=bg, material_jitter=mj)
            if fused:
                d = rs.forward_train_(batch, mat, emitter, spp, light_u, shuffle_u=shuffle_u, **kw)
                loss, _ = train_loss.fused_reference_loss(d, target, tmask, lam, mat)
                loss.backward()
            else:
                rs.forward_backward_phys(batch, target, mat, emitter, spp, light_u, shuffle_u, target_mask=tmask, loss_config=lam, **kw)
            if leaf.grad is not None:
                img.backward(leaf.grad)
            opt.step()
            sched.step()
        return step

    tr = trainer_on_bench_scene(rs, rays, mat, sg, dev, args.hw, n)
    cases = (("torch_loss", dict_step(False)), ("fused_loss", dict_step(True)), ("trainer_step", tr.step))
    res = dict(workload=f"{n} rays on the subject of the bench frame ({POSE}, {args.hw} x {args.hw}), uniform_light, spp {spp}, fwd+bwd+Adam",
               steps=args.steps, repeat=args.repeat, loss_weights={k: v for k, v in lam.items() if v})
    all_runs = timed(cases, args.steps, args.repeat)
    for name, step in cases:
        runs = all_runs[name]
        a = launch_audit.audit(step)
        res[name] = dict(ms_per_step_runs=runs, ms_per_step=sorted(runs)[len(runs) // 2], spread_ms=round(max(runs) - min(runs), 3),
                         device_launches=a["device_launches"], readbacks=a["readbacks"], idle_frac=a["idle_frac"])
        print(name, json.dumps(res[name]), flush=True)
    # (ms_per_step is the median of the repeats; the requirement: the fused route is not slower than the torch route by more than
    #  the spread of the torch route's repeats)
    res["fused_not_slower_than_torch"] = bool(res["fused_loss"]["ms_per_step"] <= res["torch_loss"]["ms_per_step"] + res["torch_loss"]["spread_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
