#!/usr/bin/env python3
"""Time isosurface(R) -- the two-pass canonical mesh export of intrinsicavatar_amd/mesh.py -- on the synthetic model.

End to end: mesh.isosurface() itself, wall clock after warm-up (median of --iters).  Split (one instrumented run of the same two passes,
device events around each stage): SDF evaluation (grid points + VolumeSDF.sdf_only, both passes), marching-cubes kernels (count, scans,
emit, faces, both passes, each including its one size read-back), host work (the rest of the wall clock).  Also vertex / face counts and
the peak allocation.  Kernel times by name: a separate `rocprofv3 --kernel-trace --stats` run of this script.

    python tools/mesh_bench.py [--resolution 512] [--chunk 2097152] [--iters 3] [--out profiles/mesh_bench_r512.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from intrinsicavatar_amd import build  # noqa: E402

DEV = "cuda:0"


def instrumented(geo, R, chunk):
    from intrinsicavatar_amd import mesh
    ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    spans = {"sdf": [], "mc": []}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bbox = geo.bbox.detach().float().cpu()
    box = (bbox[0], bbox[1])
    meshes = []
    for p in range(2):
        a, b, c = ev(), ev(), ev()
        a.record()
        level = mesh.level_grid(geo, R, box[0], box[1], chunk)
        b.record()
        m = mesh.marching_cubes(level, 0.0, box[0].tolist(), box[1].tolist())
        c.record()
        del level
        spans["sdf"].append((a, b))
        spans["mc"].append((b, c))
        meshes.append((m["v_pos"].shape[0], m["t_pos_idx"].shape[0]))
        if p == 0:
            ext = torch.stack([m["v_pos"].amin(dim=0), m["v_pos"].amax(dim=0)]).cpu()
            box = mesh.fine_bbox(ext[0], ext[1], bbox)
        del m
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    sdf = [s.elapsed_time(e) for s, e in spans["sdf"]]
    mc = [s.elapsed_time(e) for s, e in spans["mc"]]
    return dict(wall_ms=wall, sdf_ms=sdf, mc_ms=mc, host_ms=wall - sum(sdf) - sum(mc), meshes=meshes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=2097152)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    from intrinsicavatar_amd import _lib as L, mesh, synthetic as S
    rs, _, _ = S.build_frame(DEV, 16, 16, num_samples_per_ray=16, grid_D=16, grid_H=64, grid_W=64, smooth_iters=3, hash_amp=2e-3)
    geo = rs.geometry
    R = a.resolution
    mesh.isosurface(geo, R, a.chunk)                        # warm-up (code objects, allocator, hash scratch)
    torch.cuda.synchronize()
    walls = []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        out = mesh.isosurface(geo, R, a.chunk)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    nv, nf = out["v_pos"].shape[0], out["t_pos_idx"].shape[0]
    del out
    L.scratch_clear()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    mesh.isosurface(geo, R, a.chunk)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    split = instrumented(geo, R, a.chunk)
    res = dict(resolution=R, chunk=a.chunk, points_per_pass=R ** 3,
               isosurface_ms_median=round(statistics.median(walls), 2), isosurface_ms_all=[round(w, 2) for w in walls],
               target_ms=1000.0,
               split_wall_ms=round(split["wall_ms"], 2),
               sdf_eval_ms=[round(x, 2) for x in split["sdf_ms"]], mc_ms=[round(x, 3) for x in split["mc_ms"]],
               host_ms=round(split["host_ms"], 2),
               sdf_gpoints_per_s=round(2 * R ** 3 / sum(split["sdf_ms"]) / 1e6, 3),
               coarse_mesh=dict(vertices=split["meshes"][0][0], faces=split["meshes"][0][1]),
               vertices=nv, faces=nf,
               peak_alloc_gib=round(peak / 2 ** 30, 3), peak_alloc_above_baseline_gib=round((peak - base) / 2 ** 30, 3),
               device=torch.cuda.get_device_name(0), library=build.source_fingerprint())
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
