#!/usr/bin/env python3
"""Time of the three LPIPS values of ONE 540 x 540 frame (rf / pbr against the ground-truth image over valid_mask's rectangle, the aligned
albedo against the ground-truth albedo over gt_mask's) with random weights: intrinsicavatar_amd.metrics (csrc/lpips.hip, f32 MFMA) next
to the same network through torch operators on the device (the library convolution), taking turns in one process.  Reported, not gated.

    python tools/lpips_bench.py [--out profiles/lpips_frame_540.json] [--reps 7] [--warmup 2]

Two frames: the whole image (no masks) and the body-shaped mask of tools/bench_metrics.py.  Both routes run the trunk on five images (the
ground-truth image's features are formed once), in a batch of three and a batch of two, as system.evaluate_frame does.  This route reads
the rectangle on the device; the torch route is handed the rectangle as host integers, read back outside the timed region.  Times are
HIP events around one frame, median / min / max of `reps` after `warmup`; the convolution FLOP count is that of the five crops, and its
quotient by the median is given as a fraction of the 157.3 TFLOP/s f32 matrix peak of the MI355X."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

F32_PEAK_TFLOPS = 157.3


def conv_flop(h, w, convs, pool_before):
    total = 0
    for idx, cin, cout in convs:
        if idx in pool_before:
            h, w = h >> 1, w >> 1
        total += 2 * 9 * cin * cout * h * w
    return total


def device_route(M, net, f, H, W, masked):
    img = lambda t: t.reshape(H, W, 3)      # noqa: E731
    vrect = M.mask_rect(f["valid_mask"].reshape(H, W)) if masked else None
    grect = M.mask_rect((f["alpha"] > 0.5).reshape(H, W)) if masked else None
    a = M.lpips_features(net, [img(f["comp_rgb"]), img(f["comp_rgb_phys"]), img(f["rgb"])], vrect)
    b = M.lpips_features(net, [img(f["aligned"]), img(f["albedo"])], grect)
    return dict(rf_lpips=M.lpips_of_features(net, a, a, vrect, slots=(0, 2)), pbr_lpips=M.lpips_of_features(net, a, a, vrect, slots=(1, 2)),
                albedo_lpips=M.lpips_of_features(net, b, b, grect, slots=(0, 1)))


def torch_route(R, vgg, lin, f, H, W, vrect, grect):
    def crops(keys, r):
        x, y, w, h = r
        t = torch.stack([f[k].reshape(H, W, 3)[y:y + h, x:x + w] for k in keys]).permute(0, 3, 1, 2)
        return R.features(R.scaling_layer(2 * t - 1, torch.float32), vgg, torch.float32)
    a, b = crops(("rgb", "comp_rgb", "comp_rgb_phys"), vrect), crops(("albedo", "aligned"), grect)
    rgb = [t[0:1] for t in a]
    return dict(rf_lpips=R.distance([t[1:2] for t in a], rgb, lin, torch.float32).reshape(()),
                pbr_lpips=R.distance([t[2:3] for t in a], rgb, lin, torch.float32).reshape(()),
                albedo_lpips=R.distance([t[1:2] for t in b], [t[0:1] for t in b], lin, torch.float32).reshape(()))


def take_turns(routes, reps, warmup):
    """{name: fn} -> {name: (last result, [ms])}: every repetition runs each route once, in order, between two events of its own"""
    out = {k: [None, []] for k in routes}
    for i in range(warmup + reps):
        for k, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out[k][0] = fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                out[k][1].append(e0.elapsed_time(e1))
    return out


def summary(ms, reps, warmup):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=reps, warmup=warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_frame_540.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=540)
    a = ap.parse_args()
    assert a.reps >= 5 and a.warmup >= 1 and torch.cuda.is_available()
    from bench_metrics import frame
    from intrinsicavatar_amd import build, metrics as M
    from tests import lpips_ref as R
    build.build()
    dev = "cuda:0"
    H = W = a.size
    f = frame(H, W, dev)
    f["aligned"] = M.align_albedo(f["albedo"], f["comp_albedo"], f["alpha"] > 0.5)[0]
    vgg, lin = R.random_weights(0)
    net = M.LPIPSNet.from_state_dicts(vgg, lin, dev)
    vgg, lin = {k: v.to(dev) for k, v in vgg.items()}, {k: v.to(dev) for k, v in lin.items()}
    rows = {}
    for name, masked in (("whole_frame", False), ("body_mask", True)):
        vrect = M.mask_rect(f["valid_mask"].reshape(H, W)).tolist() if masked else [0, 0, W, H]
        grect = M.mask_rect((f["alpha"] > 0.5).reshape(H, W)).tolist() if masked else [0, 0, W, H]
        routes = {"this_route": lambda: device_route(M, net, f, H, W, masked)}
        torch_error = None
        try:
            torch_route(R, vgg, lin, f, H, W, vrect, grect)
            torch.cuda.synchronize()
            routes["torch_route"] = lambda: torch_route(R, vgg, lin, f, H, W, vrect, grect)
        except RuntimeError as e:                       # (the library convolution may be missing from a torch build)
            torch_error = str(e)[:300]
        got = take_turns(routes, a.reps, a.warmup)
        flop = 3 * conv_flop(vrect[3], vrect[2], M.VGG_CONVS, M.VGG_POOL_BEFORE) + 2 * conv_flop(grect[3], grect[2], M.VGG_CONVS, M.VGG_POOL_BEFORE)
        row = dict(valid_rect_xywh=vrect, gt_rect_xywh=grect, images_through_the_trunk=5, conv_flop=flop,
                   this_route_ms=summary(got["this_route"][1], a.reps, a.warmup), values_this_route=M.to_host(got["this_route"][0]))
        tf = flop / (row["this_route_ms"]["median_ms"] * 1e-3) / 1e12
        row["this_route_conv_tflops"] = tf
        row["this_route_fraction_of_f32_peak"] = tf / F32_PEAK_TFLOPS
        if "torch_route" in got:
            row["torch_route_ms"] = summary(got["torch_route"][1], a.reps, a.warmup)
            row["values_torch_route"] = {k: float(v) for k, v in got["torch_route"][0].items()}
            row["torch_route_conv_tflops"] = flop / (row["torch_route_ms"]["median_ms"] * 1e-3) / 1e12
        else:
            row["torch_route_error"] = torch_error
        rows[name] = row
    out = dict(what=f"the three LPIPS values of one {H} x {W} frame, random weights, maps on the device -> values on the device; HIP events, "
                    "the two routes taking turns in one process", device=torch.cuda.get_device_name(0),
               library_fingerprint=build.built_fingerprint(), torch=torch.__version__, f32_peak_tflops=F32_PEAK_TFLOPS, frames=rows,
               command="python tools/lpips_bench.py")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
