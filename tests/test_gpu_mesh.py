"""GPU (MI355X): the mesh export of intrinsicavatar_amd/mesh.py on csrc/mcubes.hip.

  * marching_cubes on the device == the host replay of the same arithmetic (tests/mc_harness.c), bit for bit, on analytic grids, a
    noise field that hits every cube case, non-cubic grids and all 256 single-cell cases; deterministic from run to run;
  * isosurface(geometry) on the synthetic model == the composition the reference runs: its float32 point chain on the host ->
    VolumeSDF.sdf_only in chunks -> host marching cubes -> vertex scaling, for the coarse and the fine pass, at R = 128 and 512;
    invariant to the chunk size; peak allocation at R = 512 within 3 GiB;
  * the command line writes an OBJ that parses back to the same mesh."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_mesh_cpu import _reference_fine_bbox, analytic, harness, mc_host  # noqa: F401  (harness: module fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from intrinsicavatar_amd import build
    build.build()


@pytest.fixture(scope="module")
def geometry():
    from intrinsicavatar_amd import synthetic as S
    rs, _, _ = S.build_frame(DEV, 16, 16, num_samples_per_ray=16, grid_D=16, grid_H=64, grid_W=64, smooth_iters=3, hash_amp=2e-3)
    return rs.geometry


def _gpu_mc(level, threshold=0.0, vmin=None, vmax=None):
    from intrinsicavatar_amd import mesh
    out = mesh.marching_cubes(torch.from_numpy(np.ascontiguousarray(level, np.float32)).to(DEV), threshold, vmin, vmax)
    return out["v_pos"].cpu().numpy(), out["t_pos_idx"].cpu().numpy()


def _same(got, ref, what):
    (v, f), (vr, fr) = got, ref
    assert v.shape == vr.shape and f.shape == fr.shape, (what, v.shape, vr.shape, f.shape, fr.shape)
    assert np.array_equal(f, fr), what
    assert np.array_equal(v.view(np.uint32), vr.view(np.uint32)), what


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres", "box"])
def test_analytic_grids_match_the_host_replay(harness, name):
    level, _, _ = analytic(name)
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    _same(_gpu_mc(level, 0.0, *box), mc_host(harness, level, 0.0, *box), name)
    _same(_gpu_mc(level, 0.05), mc_host(harness, level, 0.05), name + " threshold 0.05, unit box")


def test_noise_field_every_case_non_cubic_and_deterministic(harness):
    rng = np.random.default_rng(11)
    lv = rng.standard_normal((97, 61, 45)).astype(np.float32)
    ins = (-lv > 0).astype(np.int64)
    order = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
    ci = sum(ins[dx:dx + 96, dy:dy + 60, dz:dz + 44] << b for b, (dx, dy, dz) in enumerate(order))
    assert len(np.unique(ci)) == 256
    ref = mc_host(harness, lv, 0.0, (-0.3, 0.2, -2.0), (1.7, 0.9, 3.0))
    a = _gpu_mc(lv, 0.0, (-0.3, 0.2, -2.0), (1.7, 0.9, 3.0))
    b = _gpu_mc(lv, 0.0, (-0.3, 0.2, -2.0), (1.7, 0.9, 3.0))
    _same(a, ref, "noise")
    _same(b, a, "second run")
    # thin and ragged shapes (a workgroup spans several rows / slabs)
    for shape in ((2, 3, 300), (300, 2, 2), (5, 130, 7)):
        lv = rng.standard_normal(shape).astype(np.float32)
        _same(_gpu_mc(lv, 0.1), mc_host(harness, lv, 0.1), f"noise {shape}")


def test_single_cells_empty_and_full(harness):
    order = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
    for cube in range(256):
        lv = np.full((2, 2, 2), 0.75, np.float32)
        for b, c in enumerate(order):
            if cube >> b & 1:
                lv[c] = -0.5 - 0.01 * b
        _same(_gpu_mc(lv), mc_host(harness, lv), f"cube {cube}")
    for fill in (1.0, -1.0):
        v, f = _gpu_mc(np.full((9, 4, 33), fill, np.float32))
        assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == np.float32 and f.dtype == np.int64


def _reference_pass(harness, geometry, R, vmin, vmax, chunk=1 << 21):
    """isosurface_ as the reference runs it: host float32 point chain (linspace -> meshgrid ij -> scale_anything) -> forward_level
    (VolumeSDF.sdf_only of the points) in chunks -> marching cubes of -level (host replay) -> vertices scaled to (vmin, vmax)."""
    lin = torch.linspace(0, 1, R)
    sa = lambda d, lo, hi: ((d - 0) / (1 - 0)) * (hi - lo) + lo      # noqa: E731  models/utils.py scale_anything
    n = R ** 3
    level = torch.empty(n, dtype=torch.float32, device=DEV)
    for s in range(0, n, chunk):
        idx = torch.arange(s, min(s + chunk, n))
        x, y, z = lin[idx // (R * R)], lin[(idx // R) % R], lin[idx % R]
        pts = torch.stack([sa(x, vmin[0], vmax[0]), sa(y, vmin[1], vmax[1]), sa(z, vmin[2], vmax[2])], dim=-1)
        level[s:s + len(idx)] = geometry.sdf_only(pts.to(DEV))
    v, f = mc_host(harness, level.view(R, R, R).cpu().numpy(), 0.0, [float(a) for a in vmin], [float(a) for a in vmax])
    return v, f


@pytest.mark.parametrize("R", [128, 512])
def test_isosurface_matches_the_reference_composition(harness, geometry, R):
    from intrinsicavatar_amd import _lib as L, mesh
    bbox = geometry.bbox.float().cpu()
    # coarse pass
    coarse = mesh.isosurface_(geometry, bbox[0], bbox[1], R)
    ref_c = _reference_pass(harness, geometry, R, bbox.numpy()[0], bbox.numpy()[1])
    _same((coarse["v_pos"].cpu().numpy(), coarse["t_pos_idx"].cpu().numpy()), ref_c, f"coarse R={R}")
    assert len(ref_c[0]) > 1000
    del coarse
    # fine pass over the reference's expanded, clamped extent of the coarse mesh
    vmin_, vmax_ = _reference_fine_bbox(torch.from_numpy(ref_c[0]), bbox)
    ref_f = _reference_pass(harness, geometry, R, vmin_, vmax_)
    L.scratch_clear()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = mesh.isosurface(geometry, R)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    _same((out["v_pos"].cpu().numpy(), out["t_pos_idx"].cpu().numpy()), ref_f, f"fine R={R}")
    if R == 512:
        assert peak <= 3 * 2 ** 30, f"isosurface(512) peak allocation {peak / 2 ** 30:.2f} GiB"
    else:
        small = mesh.isosurface(geometry, R, chunk=1 << 18)
        assert torch.equal(small["t_pos_idx"], out["t_pos_idx"]) and torch.equal(small["v_pos"], out["v_pos"])
        geometry.isosurface_config = dict(resolution=R, chunk=1 << 20, threshold=0.0)      # the reference's model.geometry.isosurface()
        try:
            exported = mesh.export(geometry, {"export_vertex_color": True})
        finally:
            del geometry.isosurface_config
        assert torch.equal(exported["t_pos_idx"], out["t_pos_idx"]) and torch.equal(exported["v_pos"], out["v_pos"])


def test_cli_writes_the_mesh(tmp_path, geometry):
    from intrinsicavatar_amd import checkpoint, io_formats, mesh
    sd = {f"model.geometry.{k}": v.detach().cpu() for k, v in geometry.state_dict().items()}
    sd["model.occupancy_grid.binaries"] = torch.zeros(4, dtype=torch.bool)              # dropped at test time, as launch.py does
    ck = tmp_path / "last.ckpt"
    torch.save({"state_dict": sd, "global_step": 25000}, ck)
    assert set(checkpoint.split_reference_state_dict(sd)) == {"geometry"}
    bbox = geometry.bbox.float().cpu().reshape(-1).tolist()
    out = tmp_path / "mesh.obj"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "intrinsicavatar_amd.mesh", "--state-dict", str(ck),
                        "--bbox", *[repr(b) for b in bbox], "--resolution", "96", "--global-step", str(geometry.global_step),
                        "--out", str(out)], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    v, f = io_formats.load_obj(str(out))
    ref = mesh.isosurface(geometry, 96)
    assert len(v) > 100
    _same((v, f), (ref["v_pos"].cpu().numpy(), ref["t_pos_idx"].cpu().numpy()), "CLI OBJ")
