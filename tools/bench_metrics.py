#!/usr/bin/env python3
"""Time per call of the full metric set of ONE 540 x 540 frame with a body-shaped mask (rf / pbr PSNR + SSIM, normal error, albedo ratio +
aligned albedo + its PSNR + SSIM) through intrinsicavatar_amd.metrics on the device, next to the same formulas through torch on the HOST
including the copies of the maps (the reference's route: its SSIM and its mask crop leave the device).  Reported, not gated.

    python tools/bench_metrics.py [--out profiles/metrics_frame_540.json] [--iters 30] [--warmup 5]

Every timed call ends with a read-back of the metrics (device route: metrics.to_host, one copy) so that both columns measure
"maps on the device -> numbers on the host"; median of `iters` wall-clock samples after `warmup` calls."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def body_mask(H, W):
    yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    ell = lambda cy, cx, ry, rx: ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1      # noqa: E731
    m = ell(0.17, 0.5, 0.07, 0.05) | ell(0.42, 0.5, 0.2, 0.11) | ell(0.75, 0.44, 0.2, 0.045) | ell(0.75, 0.56, 0.2, 0.045)
    return m | ell(0.4, 0.33, 0.16, 0.035) | ell(0.4, 0.67, 0.16, 0.035)


def frame(H, W, dev):
    g = torch.Generator().manual_seed(0)
    n = H * W
    r = lambda *s: torch.rand(s, generator=g)      # noqa: E731
    mask = torch.from_numpy(body_mask(H, W)).reshape(n)
    rgb = r(n, 3)
    f = dict(rgb=rgb, comp_rgb=(rgb + 0.05 * (r(n, 3) - 0.5)).clamp(0, 1), comp_rgb_phys=(rgb + 0.1 * (r(n, 3) - 0.5)).clamp(0, 1),
             albedo=r(n, 3), normal=torch.randn((n, 3), generator=g), comp_normal=torch.randn((n, 3), generator=g),
             alpha=mask.float(), valid_mask=mask.clone(), w2c=torch.eye(4)[None])
    f["comp_albedo"] = (f["albedo"] * 0.8 + 0.02 * r(n, 3)).clamp(0, 1)
    return {k: v.to(dev) for k, v in f.items()}


def device_route(M, f, H, W):
    img = lambda t: t.reshape(H, W, 3)      # noqa: E731
    gm, vm = f["alpha"] > 0.5, f["valid_mask"]
    rect = M.mask_rect(vm.reshape(H, W))
    psnr = M.PSNR()
    ret = dict(rf_psnr=psnr(f["comp_rgb"], f["rgb"], valid_mask=vm), rf_ssim=M.ssim(img(f["comp_rgb"]), img(f["rgb"]), rect),
               normal_error=M.normal_error(f["comp_normal"], f["normal"], gm, w2c=f["w2c"], transform=True, normalize=True)["mean"],
               pbr_psnr=psnr(f["comp_rgb_phys"], f["rgb"], valid_mask=vm), pbr_ssim=M.ssim(img(f["comp_rgb_phys"]), img(f["rgb"]), rect))
    aligned, _ = M.align_albedo(f["albedo"], f["comp_albedo"], gm)
    ret["albedo_psnr"] = psnr(aligned, f["albedo"], valid_mask=gm)
    ret["albedo_ssim"] = M.SSIM()(img(aligned), img(f["albedo"]), valid_mask=gm.reshape(H, W))
    return M.to_host(ret)


def _host_ssim(a, b, m2d):
    """the same definition in float64 torch on the host: 7 x 7 box means over the mask's bounding rectangle, windows wholly inside."""
    rows, cols = torch.nonzero(m2d.any(1))[:, 0], torch.nonzero(m2d.any(0))[:, 0]
    y0, y1, x0, x1 = int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1
    x = a[y0:y1, x0:x1].double().permute(2, 0, 1)[None]
    y = b[y0:y1, x0:x1].double().permute(2, 0, 1)[None]
    box = lambda t: torch.nn.functional.avg_pool2d(t, 7, stride=1)      # noqa: E731
    ux, uy = box(x), box(y)
    cn = 49.0 / 48.0
    vx, vy, vxy = cn * (box(x * x) - ux * ux), cn * (box(y * y) - uy * uy), cn * (box(x * y) - ux * uy)
    C1, C2 = 0.02 ** 2, 0.06 ** 2
    return float((((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))).mean())


def host_route(f, H, W):
    h = {k: v.cpu() for k, v in f.items()}                                    # the copies are part of the route
    img = lambda t: t.reshape(H, W, 3)      # noqa: E731
    gm, vm = h["alpha"] > 0.5, h["valid_mask"]
    psnr = lambda a, b, m: float(-10 * torch.log10(torch.mean(((a - b) ** 2)[m])))      # noqa: E731
    F = torch.nn.functional
    cam = torch.matmul(h["comp_normal"], h["w2c"][0, :3, :3].T) * torch.tensor([1.0, -1.0, -1.0])
    a, b = F.normalize(cam, dim=-1), F.normalize(h["normal"], dim=-1)
    cos = (a * b).sum(-1) / (torch.linalg.norm(a, dim=-1) * torch.linalg.norm(b, dim=-1) + 1e-8)
    err = torch.rad2deg(torch.acos(cos.clamp(-1, 1)) * gm)
    x, xh = h["albedo"][gm], h["comp_albedo"][gm]
    ratio = (x * xh).sum(0) / (xh * xh).sum(0)
    aligned = torch.zeros_like(h["albedo"])
    aligned[gm] = (ratio * xh).clamp(0, 1)
    return dict(rf_psnr=psnr(h["comp_rgb"], h["rgb"], vm), rf_ssim=_host_ssim(img(h["comp_rgb"]), img(h["rgb"]), vm.reshape(H, W)),
                normal_error=float(err.sum() / gm.sum()), pbr_psnr=psnr(h["comp_rgb_phys"], h["rgb"], vm),
                pbr_ssim=_host_ssim(img(h["comp_rgb_phys"]), img(h["rgb"]), vm.reshape(H, W)), albedo_psnr=psnr(aligned, h["albedo"], gm),
                albedo_ssim=_host_ssim(img(aligned), img(h["albedo"]), gm.reshape(H, W)))


def timed(fn, iters, warmup):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), iters=iters, warmup=warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_frame_540.json"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=540)
    a = ap.parse_args()
    assert a.iters >= 20 and torch.cuda.is_available()
    from intrinsicavatar_amd import build, metrics as M
    build.build()
    H = W = a.size
    f = frame(H, W, "cuda:0")
    dev_vals, dev_t = timed(lambda: device_route(M, f, H, W), a.iters, a.warmup)
    host_vals, host_t = timed(lambda: host_route(f, H, W), a.iters, a.warmup)
    row = dict(what=f"full metric set of one {H} x {W} frame, body-shaped mask ({int(f['valid_mask'].sum())} pixels), maps on the device -> 7 numbers on the host",
               device=torch.cuda.get_device_name(0), library_fingerprint=build.built_fingerprint(), torch=torch.__version__,
               device_route_ms=dev_t, host_torch_route_ms=host_t, values_device=dev_vals, values_host=host_vals,
               command="python tools/bench_metrics.py")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(row, fh, indent=1)
        fh.write("\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
