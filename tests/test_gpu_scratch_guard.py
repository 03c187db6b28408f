"""GPU: no entry point writes past the work area its size query measured.

_lib.work_area and _lib.scan_tmp are replaced by versions that allocate 256 bytes more than asked, fill the whole buffer with 0xA5,
hand out the first `nbytes` and remember the buffer.  Every Python wrapper that owns a work area is called once at the smallest
shape that makes its layout non-trivial (one element past one tile of the entry point's own tiling) and once with one element; after a
synchronize the 256 guard bytes of every remembered buffer must still hold 0xA5, and the wrapper's outputs must equal, bit for bit,
the outputs of the same call without the patch.  The scan's callers run at one past SCAN_TILE (1025) and at one past SCAN_SMALL_MAX
(2^15): up to there one workgroup scans without touching the work area, above it the tiled protocol runs with a second level.

ia_pbr_shade_bwd reads its threshold (IA_ENV_ACC_MIN_F) once per process: its cases run in a fresh child process, which is this file
run as a program."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256


class Guarded:
    """stand-ins for _lib.work_area / _lib.scan_tmp"""

    def __init__(self, L):
        self.L, self.buffers = L, []

    def work_area(self, nbytes, device, name=None):
        nbytes = int(nbytes)
        buf = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=device)
        self.buffers.append((buf, nbytes))
        return buf[:nbytes]

    def scan_tmp(self, n, device):
        return self.work_area(int(self.L.lib().ia_scan_tmp_bytes(self.L.i64(max(int(n), 1)))) + 64, device)      # as _lib.scan_tmp

    def check(self):
        torch.cuda.synchronize()
        assert self.buffers, "the wrapper allocated no work area through _lib.work_area / _lib.scan_tmp"
        for buf, nbytes in self.buffers:
            tail = buf[nbytes:]
            assert tail.numel() == GUARD and bool((tail == 0xA5).all()), f"a work area of {nbytes} bytes was overrun"


def tensors(out):
    """the tensors of a wrapper's result, in a fixed order"""
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in tensors(o)]
    if isinstance(out, dict):
        return [t for k in sorted(out) for t in tensors(out[k])]
    if isinstance(out, (int, float, bool, str)):
        return []
    return [t for k in sorted(vars(out)) for t in tensors(getattr(out, k))]


def same_bits(a, b):
    assert len(a) == len(b) and len(a) > 0
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype
        assert torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8))


def guarded_run(case, patch):
    """case() -> result; run it plain, then with the guarded allocators (patch(name, fn) installs one)"""
    from intrinsicavatar_amd import _lib as L
    plain = [t.clone() for t in tensors(case())]
    g = Guarded(L)
    patch("work_area", g.work_area)
    patch("scan_tmp", g.scan_tmp)
    guarded = tensors(case())
    g.check()
    same_bits(plain, guarded)


@pytest.fixture
def patch(monkeypatch):
    from intrinsicavatar_amd import _lib as L
    return lambda name, fn: monkeypatch.setattr(L, name, fn)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- lib_nerfacc
SCAN_BIG = (1 << 15) + 1
RAY_COUNTS = [SCAN_BIG, 1025, 1]          # 1025: one past SCAN_TILE


def ray_lists(n_rays):
    """2 samples per ray: packed_info, interval ends, weights, sdfs"""
    rng = np.random.default_rng(n_rays)
    pi = np.stack([2 * np.arange(n_rays), np.full(n_rays, 2)], -1).astype(np.int32)
    t0 = np.sort(rng.uniform(0.1, 2.0, (n_rays, 3)).astype(np.float32), -1)
    return pi, t0, rng.uniform(0.05, 1.0, 2 * n_rays).astype(np.float32), rng.uniform(-0.1, 0.1, 2 * n_rays).astype(np.float32)


@pytest.mark.parametrize("n_rays", RAY_COUNTS)
def test_pack_info(patch, n_rays):
    from intrinsicavatar_amd import lib_nerfacc
    idx = torch.arange(n_rays, device=DEV).repeat_interleave(2)
    guarded_run(lambda: lib_nerfacc.pack_info(idx, n_rays), patch)


@pytest.mark.parametrize("n_rays", RAY_COUNTS)
def test_ray_resampling(patch, n_rays):
    from intrinsicavatar_amd import lib_nerfacc
    pi, t, w, sdf = ray_lists(n_rays)
    starts, ends = T(t[:, :2].reshape(-1, 1)), T(t[:, 1:].reshape(-1, 1))
    guarded_run(lambda: lib_nerfacc.ray_resampling(T(pi), starts, ends, T(w), T(sdf), 4), patch)


@pytest.mark.parametrize("n_rays", RAY_COUNTS)
def test_ray_resampling_merge(patch, n_rays):
    from intrinsicavatar_amd import lib_nerfacc
    _, t, w, _ = ray_lists(n_rays)
    pi = np.stack([3 * np.arange(n_rays), np.full(n_rays, 3)], -1).astype(np.int32)        # edges t0 < t1 < t2: two intervals per ray
    left = np.tile(np.array([True, True, False]), n_rays)
    right = np.tile(np.array([False, True, True]), n_rays)
    we = np.zeros((n_rays, 3), np.float32)
    we[:, :2] = w.reshape(n_rays, 2)
    guarded_run(lambda: lib_nerfacc.ray_resampling_merge(T(pi), T(t.reshape(-1)), T(left), T(right), T(we.reshape(-1)), 4), patch)


# ---------------------------------------------------------------------------------------------------------------- nerfacc
@pytest.mark.parametrize("method", ["fused", "two_pass"])
@pytest.mark.parametrize("n_rays", [257, 1])
def test_traverse_grids(patch, method, n_rays):
    from intrinsicavatar_amd import nerfacc
    rng = np.random.default_rng(5)
    binaries = T(rng.random((1, 8, 8, 8)) < 0.4)
    aabb = T(np.array([[-1, -1, -1, 1, 1, 1]], np.float32))
    o = rng.normal(size=(n_rays, 3))
    o = (3.0 * o / np.linalg.norm(o, axis=-1, keepdims=True)).astype(np.float32)
    d = rng.uniform(-0.5, 0.5, (n_rays, 3)).astype(np.float32) - o
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)

    def case():
        iv, sm, term = nerfacc.traverse_grids(T(o), T(d), binaries, aabb, None, None, 0.1, 0.0, method=method)
        return (iv.vals, iv.packed_info, iv.ray_indices, iv.is_left, iv.is_right, sm.vals, sm.packed_info, sm.ray_indices, term)
    guarded_run(case, patch)


# ---------------------------------------------------------------------------------------------------------------- hash grid
@pytest.fixture(scope="module")
def table():
    from intrinsicavatar_amd import fields
    g = torch.Generator(device=DEV).manual_seed(0)
    return (torch.rand(fields.hash_n_entries() * 2, generator=g, device=DEV) - 0.5) * 1e-2


@pytest.mark.parametrize("n", [33, 1])          # 33 x 16 levels x 8 bytes of features are no multiple of 256: the Jacobian starts behind a padded boundary
def test_hashgrid_forward_with_jacobian(patch, monkeypatch, table, n):
    from intrinsicavatar_amd import fields
    monkeypatch.setenv("IA_HASH_FWD", "xcd")
    x = T(np.random.default_rng(n).random((n, 3), dtype=np.float32))
    guarded_run(lambda: fields.hashgrid_forward(x, table, with_jac=True), patch)


@pytest.mark.parametrize("n", [129, 1025, 1])   # one past a unit (128 points), one past a workgroup's tile (1024)
def test_hashgrid_backward_binned(patch, table, n):
    from intrinsicavatar_amd import fields
    rng = np.random.default_rng(n)
    x, g_enc = T(rng.random((n, 3), dtype=np.float32)), T(rng.standard_normal((n, 32)).astype(np.float32))

    def case():
        grad = torch.zeros_like(table)
        fields.hashgrid_backward(x, g_enc, grad, method="binned")
        return grad
    guarded_run(case, patch)


# ---------------------------------------------------------------------------------------------------------------- render / deformer
@pytest.fixture(scope="module")
def frame():
    from intrinsicavatar_amd import synthetic as S
    rs, _, _ = S.build_frame(DEV, 8, 8, pose_seed=0, beta=0.01, num_samples_per_ray=16, grid_D=16, grid_H=64, grid_W=64, smooth_iters=3,
                             hash_amp=2e-3)
    return rs


def posed_points(rs, n):
    box = rs.aabbs[0].cpu().numpy()
    return T(np.random.default_rng(n).uniform(box[:3], box[3:], (n, 3)).astype(np.float32))


@pytest.mark.parametrize("n", [16385, 1])       # one past a tile of the sort
def test_morton_order(patch, frame, n):
    pts = posed_points(frame, n)
    guarded_run(lambda: frame._spatial_order(pts), patch)


@pytest.mark.parametrize("pack", ["tiles", "lookback"])
@pytest.mark.parametrize("P", [257, 1])         # one past a tile of the filter
def test_deformer_filters(patch, monkeypatch, frame, pack, P):
    monkeypatch.setenv("IA_PACK", pack)
    rng = np.random.default_rng(P)
    x = rng.uniform(-0.5, 0.5, (P, 13, 3)).astype(np.float32)
    x[:, 1::2] = x[:, 0:-1:2]                                                      # duplicates for the filter to drop
    valid = rng.random((P, 13)) < 0.6
    guarded_run(lambda: frame.deformer._pack_candidates(T(x), T(valid), with_src=True)[:4], patch)


@pytest.mark.parametrize("P", [1025, 1])        # one past a tile of the split layout
def test_deformer_rows_search(patch, frame, P):
    pts = posed_points(frame, P)
    guarded_run(lambda: frame.deformer._candidates(pts, with_src=False, split=True), patch)


# ---------------------------------------------------------------------------------------------------------------- mesh / data / metrics
@pytest.mark.parametrize("R", [3, 2])
def test_marching_cubes(patch, R):
    from intrinsicavatar_amd import mesh
    level = torch.ones((R, R, R), device=DEV)
    level[R // 2, R // 2, R // 2] = -1.0
    level[0, 0, 0] = -0.5
    guarded_run(lambda: mesh.marching_cubes(level), patch)


@pytest.mark.parametrize("hw", [(17, 17), (1, 1)])      # 289 pixels: one past a block of 256
def test_flag_lists(patch, hw):
    from intrinsicavatar_amd import data
    H, W = hw
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    mask = (((yy - H // 2) ** 2 + (xx - W // 2) ** 2) <= (min(H, W) / 3) ** 2).astype(np.float32)[None]
    smpl = dict(betas=np.zeros(10), body_pose=np.zeros((1, 69)), global_orient=np.zeros((1, 3)), transl=np.zeros((1, 3)))
    K = np.array([[20.0, 0, W / 2], [0, 20.0, H / 2], [0, 0, 1]])

    def case():
        fr = data.TrainingFrames(torch.zeros((1, H, W, 3), dtype=torch.uint8, device=DEV), T(mask), K, np.eye(4), smpl,
                                 data.EdgeSampler(10, kernel_size=5), near=0.5, far=3.0)
        return fr.mask_start, fr.edge_start, fr.counts, fr.mask_loc, fr.edge_loc
    guarded_run(case, patch)


@pytest.mark.parametrize("hw", [24, 1])
def test_ssim(patch, hw):
    from intrinsicavatar_amd import metrics
    rng = np.random.default_rng(hw)
    a, b = T(rng.random((hw, hw, 3), dtype=np.float32)), T(rng.random((hw, hw, 3), dtype=np.float32))
    guarded_run(lambda: metrics.ssim(a, b)._buf.as_subclass(torch.Tensor), patch)           # (value, status)


# ---------------------------------------------------------------------------------------------------------------- pbr (child process)
def shade_backward(F):
    from intrinsicavatar_amd import pbr
    rng = np.random.default_rng(F)
    unit = lambda v: (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)      # noqa: E731
    normal, view, out = (unit(rng.normal(size=(F, 3))) for _ in range(3))
    env = pbr.EnvironmentLightTensor(T(rng.uniform(0.2, 2.0, (16, 32, 3)).astype(np.float32)))
    env.update_pdf()
    leaves = [T(normal).requires_grad_(), T(rng.uniform(0.1, 0.9, (F, 3)).astype(np.float32)).requires_grad_(),
              T(rng.uniform(0.1, 0.9, (F, 1)).astype(np.float32)).requires_grad_(), T(rng.uniform(0.0, 1.0, (F, 1)).astype(np.float32)).requires_grad_(),
              env.base]
    env.base.grad = None
    Lo, Ld, Ls = pbr.pbr_shade_differentiable("light", leaves[0], leaves[1], leaves[2], leaves[3], T(view), T(out),
                                              T(rng.uniform(0.0, 1.0, (F, 1)).astype(np.float32)), None, env, T(np.eye(3, dtype=np.float32)))
    (Lo.sum() + 0.5 * Ld.sum() + 0.25 * Ls.sum()).backward()
    return [t.grad for t in leaves]


def child_main():
    from intrinsicavatar_amd import _lib as L
    assert os.environ.get("IA_ENV_ACC_MIN_F") == "1"
    for F in (8193, 1):                          # one past a tile of the band sort
        assert int(L.lib().ia_pbr_shade_bwd_scratch_bytes(L.i64(F))) > 0
        saved = (L.work_area, L.scan_tmp)
        try:
            guarded_run(lambda: shade_backward(F), lambda name, fn: setattr(L, name, fn))
        finally:
            L.work_area, L.scan_tmp = saved
    print("shade backward guard OK")


def test_pbr_shade_backward_in_a_fresh_process():
    env = dict(os.environ, IA_ENV_ACC_MIN_F="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "shade-backward-child"], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0 and "shade backward guard OK" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


if __name__ == "__main__" and sys.argv[1:] == ["shade-backward-child"]:
    child_main()
