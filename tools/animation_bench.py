#!/usr/bin/env python3
"""Animation / relighting test path: a synthetic model over AIST animation frames (the committed frames 0 / 100 / 200 / 319 of the
reference's load/animation/aist/poses.npz, plain FK), 540 x 540 rays, render_mode light -- once with a constant background and once with
the emitter behind the avatar (add_emitter) -- plus the time of ia_envlight_background alone at 540 x 540 rays on a 1024 x 2048 map.

    python tools/animation_bench.py                                      -> profiles/animation_sequence.json, key "tree"
    python tools/animation_bench.py --package-root DIR --label parent    the same frames through the package of another checkout (one
                                                                         without add_emitter runs the constant background only); merged
                                                                         into the same file under "parent"

A frame pays what the reference's animation loop pays per frame (synthetic.repose: bone transforms -> skinning grids -> occupancy grid from
the model) inside the timed region; one untimed pass over the distinct poses first (device allocations done)."""
import argparse, inspect, json, os, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--hw", type=int, default=540)
ap.add_argument("--spp", type=int, default=256)
ap.add_argument("--frames", type=int, default=4)
ap.add_argument("--gi", action="store_true")
ap.add_argument("--package-root", default=ROOT)
ap.add_argument("--label", default="tree")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "animation_sequence.json"))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package_root))
from intrinsicavatar_amd import build
build.build()
from intrinsicavatar_amd import synthetic as S, fields, pbr, render, _lib as L

dev = "cuda:0"
hw, spp = args.hw, args.spp
has_emitter = "add_emitter" in inspect.signature(render.RenderStep.relight).parameters
mat = fields.VolumeMaterial(seed=2).to(dev)
H, W = 1024, 2048
v, u = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
img = np.where((v < 0.5)[..., None], np.stack([0.3 + 0.4 * (1 - v), 0.4 + 0.4 * (1 - v), 0.6 + 0.4 * (1 - v)], -1), 0.08)
img = img + (30.0 * np.exp(-(((u - 0.3) * 2) ** 2 + ((v - 0.25) * 2) ** 2) / (2 * 0.02 ** 2)))[..., None]
env = pbr.EnvironmentLightTensor(torch.from_numpy(img.astype(np.float32)).to(dev))
env.update_pdf()
g = torch.Generator().manual_seed(0)
light_u = torch.rand((spp, 3), generator=g).to(dev)            # resample_light false: one set for the sequence
AIST = (0, 100, 200, 319)
pose_of = lambda k: f"aist:{AIST[k % len(AIST)]}"              # noqa: E731
rs, rays, _ = S.build_frame(dev, hw, hw, pose=pose_of(0), beta=0.01)
shuffle_u = torch.rand((rays.shape[0], spp), generator=g).to(dev)      # host generator: the same numbers in every process


def frame(k, add_emitter):
    S.repose(rs, pose_of(k))
    kw = dict(add_emitter=True) if add_emitter else {}
    o = rs.relight(rays, mat, env, spp, light_u, shuffle_u, global_illumination=args.gi, **kw)
    return o["stats"]


def timed(add_emitter):
    for k in range(min(len(AIST), args.frames)):
        frame(k, add_emitter)
    times, stats = [], None
    for k in range(args.frames):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = frame(k, add_emitter)
        torch.cuda.synchronize()
        times.append(round(time.perf_counter() - t0, 4))
    return dict(s_per_frame=times, s_per_frame_mean=round(float(np.mean(times)), 4), n_fg_last=int(stats["n_fg"]), n_secondary_last=int(stats["n_secondary"]))


res = dict(hw=hw, spp=spp, gi=bool(args.gi), frames=args.frames, poses=[pose_of(k) for k in range(args.frames)], env=[H, W],
           add_emitter_false=timed(False))
if has_emitter:
    res["add_emitter_true"] = timed(True)
    # the kernel alone: one launch per frame's rays, timed with events over 50 launches after 5 untimed ones
    d = rs.deformer.transform_rays_w2s(rays.float())[:, 3:6].contiguous()
    rot = rs.deformer.w2s[:3, :3].contiguous()
    for _ in range(5):
        env.background(d, rot)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        env.background(d, rot)
    e1.record()
    torch.cuda.synchronize()
    res["ia_envlight_background_us_540x540"] = round(e0.elapsed_time(e1) / 50 * 1e3, 2)
    res["ia_envlight_background_note"] = "wall time per call between two events, launch and output allocation included; 291 600 rays, 1024 x 2048 map"
os.makedirs(os.path.dirname(args.out), exist_ok=True)
allr = json.load(open(args.out)) if os.path.exists(args.out) else {}
allr[args.label] = res
json.dump(allr, open(args.out, "w"), indent=1)
print(json.dumps({args.label: res}))
