#!/usr/bin/env python3
"""Time forward skinning and the vertex normals on the R = 512 mesh of the synthetic model -> profiles/mesh_pose.json.

    python tools/mesh_pose_bench.py [--resolution 512] [--iters 20] [--out profiles/mesh_pose.json]

One process, one library: the canonical mesh (mesh.isosurface at R), then, on its vertices,
    kernel      ia_forward_skinning (csrc/lbs_fwd.hip) for xd + R (what the reference's forward_skinning returns), for the weights
                alone (query_weights), and for all three outputs
    torch       the same values through torch.nn.functional.grid_sample + the [P,24] x [24,16] product + the point transform
                (the expressions SNARFDeformer.query_weights / implicit_pose_terms used before the kernel)
    normals     mesh.vertex_normals (count, scan, fill, sort + sum: csrc/mesh_attr.hip) and mesh.pose as a whole
each as the median of --iters device-event timings after a warm-up, on two weight grids: the synthetic model's own and a [24,32,128,128]
grid (resolution 128, what SNARFDeformer.from_smpl builds) with the same box.  Rates: compulsory bytes (12 B read per point, the
outputs written once) against the measured HBM copy rate, and gathered bytes (24 channels x 8 corners x 4 B per point, served by the
caches) against the L2 rate -- the figures of the MI355X micro-architecture notes (6.29 TB/s, 34.5 TB/s).  The difference between the
kernel and the torch path is reported as a maximum, not asserted.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
HBM_BPS = 6.29e12          # measured float4 copy
L2_BPS = 34.5e12           # aggregate L2


def timed(fn, iters):
    fn()
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


@torch.no_grad()
def torch_path(d, xc):
    g = ((xc + d.offset_kernel) * d.scale_kernel).reshape(1, -1, 1, 1, 3)
    w = torch.nn.functional.grid_sample(d.lbs_voxel_final, g, align_corners=True, mode="bilinear", padding_mode="border")
    w = w.reshape(w.shape[1], -1).t()
    T = (w @ d.tfs[0].reshape(24, 16)).reshape(-1, 4, 4)
    R = T[:, :3, :3]
    xd = (R * xc[:, None, :]).sum(-1) + T[:, :3, 3]
    return xd, R, w


def one_grid(d, v, iters):
    P = v.shape[0]
    res = dict(grid=list(d.lbs_voxel_final.shape[1:]), grid_mib=round(d.lbs_voxel_final.numel() * 4 / 2 ** 20, 1))
    cases = {"xd_R": dict(want_weights=False, want_xd=True, want_rot=True, out_bytes=48),
             "w": dict(want_weights=True, want_xd=False, want_rot=False, out_bytes=96),
             "w_xd_R": dict(want_weights=True, want_xd=True, want_rot=True, out_bytes=144)}
    for name, c in cases.items():
        out_bytes = c.pop("out_bytes")
        med, lo, hi = timed(lambda: d._lbs(v, c["want_weights"], c["want_xd"], c["want_rot"]), iters)
        compulsory, gathered = P * (12 + out_bytes), P * 24 * 8 * 4
        res[f"kernel_{name}_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
        res[f"kernel_{name}_rates"] = dict(
            points_per_s=round(P / med * 1e3), compulsory_bytes=compulsory, compulsory_tb_per_s=round(compulsory / med / 1e9, 3),
            share_of_hbm_copy_rate=round(compulsory / med * 1e3 / HBM_BPS, 3), gathered_bytes=gathered,
            gathered_tb_per_s=round(gathered / med / 1e9, 3), share_of_l2_rate=round(gathered / med * 1e3 / L2_BPS, 3))
    med, lo, hi = timed(lambda: torch_path(d, v), iters)
    res["torch_grid_sample_product_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
    res["torch_over_kernel_w_xd_R"] = round(med / res["kernel_w_xd_R_ms"]["median"], 2)
    xd, R, w = d._lbs(v, True, True, True)
    txd, tR, tw = torch_path(d, v)
    res["max_abs_difference_to_torch"] = dict(w=float((w - tw).abs().max()), xd=float((xd - txd).abs().max()), R=float((R - tR).abs().max()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_pose_bench needs the MI355X: a time measured elsewhere says nothing about it")
    from intrinsicavatar_amd import build, mesh, synthetic as S
    from intrinsicavatar_amd.deformer import SNARFDeformer
    rs, _, _ = S.build_frame(DEV, 16, 16, num_samples_per_ray=16, grid_D=16, grid_H=64, grid_W=64, smooth_iters=3, hash_amp=2e-3)
    m = mesh.isosurface(rs.geometry, a.resolution)
    v, f = m["v_pos"], m["t_pos_idx"]
    d0 = rs.deformer
    gen = torch.Generator(device=DEV).manual_seed(0)
    big = torch.rand((1, 24, 32, 128, 128), device=DEV, generator=gen) + 0.05
    big = big / big.sum(1, keepdim=True)
    d1 = SNARFDeformer(big, d0.offset_kernel, d0.scale_kernel, d0.bbox)
    d1.tfs = d0.tfs
    res = dict(resolution=a.resolution, vertices=int(v.shape[0]), faces=int(f.shape[0]), iters=a.iters,
               hbm_copy_rate_tb_per_s=HBM_BPS / 1e12, l2_rate_tb_per_s=L2_BPS / 1e12,
               model_grid=one_grid(d0, v, a.iters), resolution_128_grid=one_grid(d1, v, a.iters))
    med, lo, hi = timed(lambda: mesh.vertex_normals(v, f), a.iters)
    res["vertex_normals_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
    med, lo, hi = timed(lambda: mesh.pose(m, d0), a.iters)
    res["pose_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
    valence = torch.diff(mesh.vertex_faces(v.shape[0], f)[0])
    res["valence"] = dict(max=int(valence.max()), mean=round(float(valence.float().mean()), 2))
    res.update(device=torch.cuda.get_device_name(0), library=build.source_fingerprint())
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
