"""Golden vectors for forward skinning (grid lookup of the skinning weights + blend of the bone transforms) and a small fixture mesh
for the vertex normals.

Runs ONLY where /root/reference exists.  It imports the reference's own `ForwardDeformer.switch_to_explicit` -- whose `query_weights`
closure is the operator under test -- and `skinning_mask` (models/deformers/fast_snarf/deformer_torch.py:139-227) and runs them on the
CPU through a stand-in object: `switch_to_explicit(use_smpl=False)` takes the grid from `self.query_weights`, which the stand-in
answers with the fixture's grid, and then installs the closure that samples it.  The three JIT CUDA extensions deformer_torch.py loads
at import are stubbed out as in make_golden_skinning.py (none of them is called here).
    python tests/golden/make_golden_lbs.py      ->  tests/golden/golden_lbs.npz, golden_lbs_w.npz   (arrays only)

    golden_lbs.npz      grid [1,24,4,16,16] (positive, normalised over the channels), offset_kernel / scale_kernel [3] (z scale x 4 as
                        switch_to_explicit makes it), bbox [2,3], tfs [24,4,4] (random rigid), xc [4096,3] + kind [4096] (0 interior,
                        1 on a grid node, 2 on the last node of an axis, 3 outside one side, 4 one point per face / edge / corner
                        region outside the box), the reference's xd [4096,3] and R [4096,3,3]; mesh_v / mesh_f: a marching-cubes
                        sphere at 8^3 (the product's own host extraction, tests/mc_harness.c) + a 12-face fan (one vertex of valence
                        12) + one zero-area face; mesh_n_sphere = number of sphere vertices
    golden_lbs_w.npz    the reference's w [4096,24]
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

D, H, W = 4, 16, 16
P = 4096


def rigid_tfs(rng):
    from intrinsicavatar_amd import smpl
    aa = torch.from_numpy(rng.normal(size=(24, 3)) * 0.6)
    T = torch.zeros((24, 4, 4), dtype=torch.float64)
    T[:, :3, :3] = smpl.rodrigues(aa)
    T[:, :3, 3] = torch.from_numpy(rng.normal(size=(24, 3)) * 0.3)
    T[:, 3, 3] = 1.0
    return T.float().numpy()


def points(rng, denormalize):
    """normalised coordinates n in (and around) [-1, 1]^3 -> canonical points through the reference's own denormalize"""
    n, kind = [], []
    n.append(rng.uniform(-1, 1, size=(P - 600 - 300 - 600 - 26, 3)))                    # interior
    kind += [0] * len(n[-1])
    node = np.stack([np.linspace(-1, 1, W)[rng.integers(0, W, 600)], np.linspace(-1, 1, H)[rng.integers(0, H, 600)],
                     np.linspace(-1, 1, D)[rng.integers(0, D, 600)]], 1)                 # on grid nodes (all three axes)
    half = rng.random((600, 3)) < 0.3                                                    # ... some axes between nodes
    node = np.where(half, rng.uniform(-1, 1, size=(600, 3)), node)
    n.append(node)
    kind += [1] * 600
    last = rng.uniform(-1, 1, size=(300, 3))                                             # the last node of each axis
    for i in range(300):
        last[i, i % 3] = 1.0
        if i % 7 == 0:
            last[i, (i + 1) % 3] = 1.0
    n.append(last)
    kind += [2] * 300
    out = rng.uniform(-1, 1, size=(600, 3))                                              # outside, every side
    for i in range(600):
        a, s = (i // 2) % 3, 1.0 if i % 2 else -1.0
        out[i, a] = s * (1.0 + rng.uniform(1e-3, 0.8))
    n.append(out)
    kind += [3] * 600
    reg = []
    for sx in (-1, 0, 1):                                                                # one point per face, edge and corner region
        for sy in (-1, 0, 1):
            for sz in (-1, 0, 1):
                if (sx, sy, sz) != (0, 0, 0):
                    r = rng.uniform(-0.9, 0.9, 3)
                    reg.append([s * 1.3 if s else r[k] for k, s in enumerate((sx, sy, sz))])
    n.append(np.array(reg))
    kind += [4] * 26
    n = torch.from_numpy(np.concatenate(n).astype(np.float32))
    assert n.shape == (P, 3)
    return denormalize(n[None])[0].contiguous(), np.array(kind, np.int8)


def fixture_mesh():
    """(mesh_v float32 [V,3], mesh_f int64 [T,3], number of sphere vertices)"""
    tmp = tempfile.mkdtemp(prefix="golden_lbs_")
    so = os.path.join(tmp, "libmc_harness.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-fvisibility=hidden", "-o", so,
                           os.path.join(os.path.dirname(HERE), "mc_harness.c"), "-lm"])
    h = C.CDLL(so)
    ax = np.linspace(-1, 1, 8)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    lv = np.ascontiguousarray(np.sqrt(X ** 2 + Y ** 2 + Z ** 2) - 0.6, dtype=np.float32)
    cnt = np.zeros(2, np.int64)
    vp = C.c_void_p
    h.mc_h_count(C.c_int(8), C.c_int(8), C.c_int(8), vp(lv.ctypes.data), C.c_float(0.0), vp(cnt.ctypes.data))
    v = np.zeros((int(cnt[0]), 3), np.float32)
    f = np.zeros((int(cnt[1]), 3), np.int64)
    box = np.array([-1, -1, -1, 1, 1, 1], np.float32)
    assert h.mc_h_fill(C.c_int(8), C.c_int(8), C.c_int(8), vp(lv.ctypes.data), C.c_float(0.0), vp(box.ctypes.data), vp(v.ctypes.data),
                       vp(f.ctypes.data)) == 0
    n_sphere = len(v)
    # a fan of 12 faces around an apex above the sphere (counter-clockwise seen from +z: normals point up)
    ang = np.arange(12) * (2 * np.pi / 12)
    ring = np.stack([0.3 * np.cos(ang), 0.3 * np.sin(ang), np.full(12, 0.9)], 1).astype(np.float32)
    apex = n_sphere
    v = np.concatenate([v, np.array([[0.0, 0.0, 0.97]], np.float32), ring])
    fan = np.array([[apex, apex + 1 + k, apex + 1 + (k + 1) % 12] for k in range(12)], np.int64)
    degenerate = np.array([[5, 5, 9]], np.int64)                                         # zero area, one vertex twice
    f = np.concatenate([f[: len(f) // 2], degenerate, f[len(f) // 2:], fan])
    return v, f, n_sphere


def main():
    import make_golden_skinning as MS
    dt, _ = MS.load_reference(None)
    rng = np.random.default_rng(23)
    grid = rng.random((1, 24, D, H, W)).astype(np.float32) + 0.05
    grid = torch.from_numpy(grid)
    grid = grid / grid.sum(1, keepdim=True)

    d = dt.ForwardDeformer.__new__(dt.ForwardDeformer)
    torch.nn.Module.__init__(d)
    d.global_scale = 1.2
    d.device = "cpu"
    d.query_weights = lambda x, cond, mask: grid                        # switch_to_explicit(use_smpl=False) asks the object for its grid
    verts = torch.tensor([[[-0.45, -0.93, -0.12], [0.57, 0.81, 0.21], [0.1, 0.2, 0.05]]], dtype=torch.float32)
    d.switch_to_explicit(resolution=H, smpl_verts=verts, use_smpl=False)
    assert d.lbs_voxel_final.shape == (1, 24, D, H, W) and d.ratio == 4.0
    assert torch.equal(d.lbs_voxel_final, grid)

    xc, kind = points(rng, d.denormalize)
    tfs = rigid_tfs(rng)
    with torch.no_grad():
        w = d.query_weights(xc[None])[0]                                # the closure switch_to_explicit installed
        xd, R = dt.skinning_mask(xc, w, torch.from_numpy(tfs)[None])
    assert w.shape == (P, 24) and xd.shape == (P, 3) and R.shape == (P, 3, 3)
    mesh_v, mesh_f, n_sphere = fixture_mesh()

    np.savez_compressed(os.path.join(HERE, "golden_lbs.npz"), grid=grid.numpy(), offset_kernel=d.offset_kernel.numpy().reshape(3),
                        scale_kernel=d.scale_kernel.numpy().reshape(3), bbox=d.bbox.numpy(), tfs=tfs, xc=xc.numpy(), kind=kind,
                        xd=xd.numpy(), R=R.numpy(), mesh_v=mesh_v, mesh_f=mesh_f.astype(np.int32), mesh_n_sphere=np.int32(n_sphere))
    np.savez_compressed(os.path.join(HERE, "golden_lbs_w.npz"), w=w.numpy())
    for f in ("golden_lbs.npz", "golden_lbs_w.npz"):
        p = os.path.join(HERE, f)
        print(p, os.path.getsize(p))
        assert os.path.getsize(p) < (1 << 19), p
    print("kinds:", np.bincount(kind), "mesh:", mesh_v.shape, mesh_f.shape, "sphere vertices:", n_sphere)


if __name__ == "__main__":
    main()
