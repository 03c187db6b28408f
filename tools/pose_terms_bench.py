#!/usr/bin/env python3
"""Time the backward of the pose terms, parent route against the fused node -> profiles/pose_terms.json.

    python tools/pose_terms_bench.py [--points 400000] [--iters 50] [--out profiles/pose_terms.json]

The samples of a posed synthetic frame (128 x 128 rays of synthetic.build_frame on the [24,32,128,128] weight grid, the resolution
SNARFDeformer.from_smpl builds): the winners' canonical points, inverse Jacobians and validity flags as train.shade_front hands
them to the pose terms, repeated up to --points rows (the 4096-ray training batch has about 4e5), with random gradients for
pts_cano and c2w.  One process, the two routes taking turns, --iters rounds after a warm-up, device events around each call:

    parent   SNARFDeformer.implicit_pose_terms + `c2w + (R - R.detach()) * valid` + torch.autograd.backward: ia_forward_skinning for
             the weights [P,24], the [P,24] x [24,16] library product, the ATen chain, and their mirrors in backward
    node     SNARFDeformer.pose_terms (deformer._PoseTerms) + torch.autograd.backward: nothing in forward, ia_pose_terms_bwd in backward

and, per route, the device launches of ONE call counted as tools/launch_audit.py counts them (the device events of torch.profiler)
and the time of this library's entry points alone (the binding's events around each: ia_forward_skinning of the parent route,
ia_pose_terms_bwd of the node) -- the rest of a route's time is ATen / library kernels and the host between launches.
Parity: both routes against fp64 CPU autograd of the same expressions at the sizes of tests/test_gpu_pose_terms.py and at --points.
Nothing is asserted; what is measured is written down.
"""
import argparse
import collections
import json
import os
import statistics
import sys

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"


def frame_samples(rs, rays, points, gen):
    """(xc, c2w, J_inv, valid) of the frame's samples, as train.shade_front gathers them, repeated to `points` rows"""
    from intrinsicavatar_amd import render
    with torch.no_grad():
        rays_o, rays_d, _, t_starts, t_ends, ray_indices, _, _ = rs.sample(rays)
        pts = render.ray_points(rays_o, rays_d, ray_indices, t_starts, t_ends)
        d = rs.deformer.deform(pts, rs.geometry, with_grad=False, with_feature=False, want_fwd=True, want_jinv=True)
        win = d["cand_src"].long()[d["sel"].long().clamp(min=0)]
        xc, valid = d["pts_cano"], d["valid"]
        c2w, J_inv = d["fwd_J"].reshape(-1, 3, 3)[win], d["J_inv"].reshape(-1, 3, 3)[win]
        n = xc.shape[0]
        rep = torch.arange(points, device=xc.device) % n
        return n, xc[rep].contiguous(), c2w[rep].contiguous(), J_inv[rep].contiguous(), valid[rep].contiguous()


def routes(dfm, xc, c2w, J_inv, valid, g_pts, g_c2w):
    def parent():
        dfm.tfs.grad = None
        pts, R = dfm.implicit_pose_terms(xc, J_inv, valid)
        c2 = c2w + (R - R.detach()) * valid[:, None, None].to(R.dtype)
        torch.autograd.backward([pts, c2], [g_pts, g_c2w])
        return dfm.tfs.grad

    def node():
        dfm.tfs.grad = None
        pts, c2 = dfm.pose_terms(xc, c2w, J_inv, valid)
        torch.autograd.backward([pts, c2], [g_pts, g_c2w])
        return dfm.tfs.grad
    return dict(parent=parent, node=node)


def launches(fn):
    from torch.profiler import profile, ProfilerActivity
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    dev = [e for e in prof.events() if getattr(e, "device_type", None) is not None and str(e.device_type).endswith("CUDA")]
    names = collections.Counter(e.name[:90] for e in dev)
    return dict(device_launches=len(dev), by_name=names.most_common())


def fp64_reference(dfm, xc, c2w, J_inv, valid, g_pts, g_c2w):
    D = lambda t: t.detach().cpu().double()      # noqa: E731
    w, tfs = D(dfm.query_weights(xc)), D(dfm.tfs[0]).requires_grad_(True)
    x, Ji, v = D(xc), D(J_inv), D(valid)
    T = (w @ tfs.reshape(24, 16)).reshape(-1, 4, 4)
    R = T[:, :3, :3]
    xd = (R * x[:, None, :]).sum(-1) + T[:, :3, 3]
    corr = -(Ji * (xd - xd.detach())[:, None, :]).sum(-1) * v[:, None]
    torch.autograd.backward([x + corr, D(c2w) + (R - R.detach()) * v[:, None, None]], [D(g_pts), D(g_c2w)])
    return tfs.grad


def parity(dfm, P, gen):
    lo, hi = dfm.bbox[0], dfm.bbox[1]
    r = lambda *s: torch.randn(s, device=DEV, generator=gen)      # noqa: E731
    xc = ((lo + hi) / 2 + (torch.rand((P, 3), device=DEV, generator=gen) - 0.5) * 1.4 * (hi - lo)).contiguous()
    valid = torch.rand(P, device=DEV, generator=gen) >= 0.3
    args = (xc, r(P, 3, 3), r(P, 3, 3), valid, r(P, 3), r(P, 3, 3))
    want = fp64_reference(dfm, *args)
    out = {k: float((f()[0].cpu().double() - want).abs().max()) for k, f in routes(dfm, *args).items()}
    return dict(points=P, largest_entry=float(want.abs().max()), max_abs_error_parent=out["parent"], max_abs_error_node=out["node"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=400000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_terms_bench needs the MI355X: a time measured elsewhere says nothing about it")
    from intrinsicavatar_amd import build, synthetic as S
    build.build()
    rs, rays, _ = S.build_frame(DEV, 128, 128, pose_seed=0, beta=0.02, num_samples_per_ray=128, smooth_iters=5, hash_amp=2e-3)
    dfm = rs.deformer
    gen = torch.Generator(device=DEV).manual_seed(0)
    n_frame, xc, c2w, J_inv, valid = frame_samples(rs, rays, a.points, gen)
    P = xc.shape[0]
    g_pts, g_c2w = torch.randn((P, 3), device=DEV, generator=gen), torch.randn((P, 3, 3), device=DEV, generator=gen)
    dfm.tfs = dfm.tfs.detach().clone().requires_grad_(True)
    fns = routes(dfm, xc, c2w, J_inv, valid, g_pts, g_c2w)
    for _ in range(3):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(a.iters):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    res = dict(points=P, frame_samples=n_frame, valid_fraction=round(float(valid.float().mean()), 4), iters=a.iters,
               grid=list(dfm.lbs_voxel_final.shape[1:]),
               ms={k: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in ms.items()})
    res["parent_over_node"] = round(res["ms"]["parent"]["median"] / res["ms"]["node"]["median"], 2)
    # the entry points alone (the binding's own events, no host time between them): what of each route is kernel time of this library
    from intrinsicavatar_amd import _lib as L
    abi = {}
    for k, f in fns.items():
        per_call = collections.defaultdict(list)
        for _ in range(a.iters):
            L.lib().start()
            f()
            for name, (_, total) in L.lib().report().items():
                per_call[name].append(total)
        abi[k] = {name: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4)) for name, v in per_call.items()}
    res["entry_point_ms"] = abi
    res["launches"] = {k: launches(f) for k, f in fns.items()}
    want = fp64_reference(dfm, xc, c2w, J_inv, valid, g_pts, g_c2w)
    res["parity_frame"] = dict(points=P, largest_entry=float(want.abs().max()),
                               **{"max_abs_error_" + k: float((f()[0].cpu().double() - want).abs().max()) for k, f in fns.items()})
    res["parity_random"] = [parity(dfm, p, gen) for p in (1, 63, 65, 257, 4099)]
    a_, b_ = fns["node"]().clone(), fns["node"]().clone()
    res["node_bit_identical_twice"] = bool(torch.equal(a_.view(torch.int32), b_.view(torch.int32)))
    res.update(device=torch.cuda.get_device_name(0), library=build.source_fingerprint())
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
