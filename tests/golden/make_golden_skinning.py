"""Golden vectors for building the deformer from a body surface (voxel centres, k-NN, inverse-distance blend, smoothing sweeps).

Runs ONLY where /root/reference exists.  It imports the reference's own `ForwardDeformer.switch_to_explicit` / `query_weights_smpl`
(models/deformers/fast_snarf/deformer_torch.py:139-253) and `get_predefined_rest_pose` / `get_bbox_from_smpl`
(models/deformers/snarf_deformer.py:9-35) and runs them on the CPU.  `ops.knn_points` is bound to the reference's own
lib/pytorch3d/cuda/knn_cpu.cpp, compiled at generation time into a scratch directory with -ffp-contract=off (nothing of it is
committed); the three JIT CUDA extensions deformer_torch.py loads at import are stubbed out (none of them is called here).
    python tests/golden/make_golden_skinning.py      ->  tests/golden/golden_skinning*.npz   (data only)

torch.linspace is pinned while the reference runs: its CPU kernel evaluates the two-sided formula (start + i * step below the midpoint,
end - (steps - 1 - i) * step from it on) in SIMD chunks as chunk_base + lane * step, so its float32 values depend on the vector width
of the host that runs it (AVX2 and AVX-512 hosts disagree by an ulp on some elements).  Here every element is evaluated with the scalar
form of that formula -- the expression of torch's CUDA kernel and of the CPU kernel's scalar tail -- which is what csrc/skin_math.h
evaluates.  `linspace_host_diffs` in the fixture records on how many elements this host's own torch.linspace differs.

The body: a seeded synthetic surface on the capsule skeleton of intrinsicavatar_amd/synthetic.py, V = 6890, at most 4 non-zero skinning
weights per vertex (stored sparsely), and a handful of exactly duplicated vertices so that equal distances occur.

The fixture is split into parts so that every committed file stays below 1 MiB:
    golden_skinning.npz         body, offset / scale / bbox, grid points, idx (K = 30), small k-NN cases, resolution-128 sample, smpl helpers
    golden_skinning_d2.npz      d2 of the resolution-32 grid (K = 30)
    golden_skinning_blend.npz   blended weights [24, 8192] and the grid after 1 sweep
    golden_skinning_grid.npz    the grid after 30 sweeps
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

V = 6890
K = 30


def build_knn_cpu(tmp):
    from torch.utils import cpp_extension
    wrap = os.path.join(tmp, "knn_wrap.cpp")
    with open(wrap, "w") as fh:
        fh.write('#include "%s/lib/pytorch3d/cuda/knn_cpu.cpp"\n'
                 'PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) { m.def("knn", &KNearestNeighborIdxCpu); }\n' % REF)
    return cpp_extension.load(name="ref_knn_cpu", sources=[wrap], extra_cflags=["-O2", "-ffp-contract=off"], build_directory=tmp,
                              verbose=False)


def load_reference(knn_ext):
    from collections import namedtuple
    KNN = namedtuple("KNN", "dists idx knn")

    def knn_points(p1, p2, lengths1=None, lengths2=None, norm=2, K=1, version=-1, return_nn=False, return_sorted=True):
        p1, p2 = p1.contiguous().float(), p2.contiguous().float()
        l1 = torch.full((p1.shape[0],), p1.shape[1], dtype=torch.int64)
        l2 = torch.full((p2.shape[0],), p2.shape[1], dtype=torch.int64)
        idx, d = knn_ext.knn(p1, p2, l1, l2, norm, K)
        return KNN(d, idx, None)

    lib = types.ModuleType("lib")
    p3d = types.ModuleType("lib.pytorch3d")
    ops = types.ModuleType("lib.pytorch3d.ops")
    ops.knn_points = knn_points
    p3d.ops, lib.pytorch3d = ops, p3d
    sys.modules.update({"lib": lib, "lib.pytorch3d": p3d, "lib.pytorch3d.ops": ops})
    from torch.utils import cpp_extension
    real_load = cpp_extension.load
    cpp_extension.load = lambda **kw: None                      # fuse_cuda / filter / precompute: CUDA sources, never called here
    try:
        def load(name, path, package=None):
            spec = importlib.util.spec_from_file_location(name, path)
            mod = importlib.util.module_from_spec(spec)
            if package:
                mod.__package__ = package
            sys.modules[name] = mod
            spec.loader.exec_module(mod)
            return mod
        dt = load("refdef.fast_snarf.deformer_torch", f"{REF}/models/deformers/fast_snarf/deformer_torch.py")
        for name in ("refdef", "refdef.fast_snarf", "refdef.smplx", "torchgeometry", "torchgeometry.core", "torchgeometry.core.conversions"):
            sys.modules.setdefault(name, types.ModuleType(name))
        sys.modules["refdef"].__path__ = []
        sys.modules["refdef.fast_snarf"].__path__ = []
        sys.modules["refdef.smplx"].SMPL = object
        sys.modules["torchgeometry"].__path__ = []
        sys.modules["torchgeometry.core"].__path__ = []
        sys.modules["torchgeometry.core"].conversions = sys.modules["torchgeometry.core.conversions"]
        sd = load("refdef.snarf_deformer", f"{REF}/models/deformers/snarf_deformer.py", package="refdef")
    finally:
        cpp_extension.load = real_load
    return dt, sd


def scalar_linspace(start, end, steps, device=None, **kw):
    f = np.float32
    start, end = f(start), f(end)
    step = (end - start) / f(steps - 1)
    out = np.array([start + step * f(i) if i < steps // 2 else end - step * f(steps - i - 1) for i in range(steps)], np.float32)
    return torch.from_numpy(out)


def make_body(seed=11):
    """(verts [V,3] float32, w_idx [V,4] int8, w_val [V,4] float32): points on the capsule surfaces of the stick figure."""
    from intrinsicavatar_amd import synthetic as S
    rng = np.random.default_rng(seed)
    bone = rng.integers(1, 24, V)
    a, b = S.JOINTS[S.PARENTS[bone]], S.JOINTS[bone]
    t = rng.random(V).astype(np.float32)
    u = rng.normal(size=(V, 3)).astype(np.float32)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = S.RADII[S.PARENTS[bone]] + (S.RADII[bone] - S.RADII[S.PARENTS[bone]]) * t
    verts = (a + t[:, None] * (b - a) + r[:, None] * u).astype(np.float32)
    w_idx = np.stack([bone, S.PARENTS[bone], rng.integers(0, 24, V), rng.integers(0, 24, V)], 1).astype(np.int8)
    w_val = rng.random((V, 4)).astype(np.float32) * np.array([1.0, 0.6, 0.2, 0.1], np.float32)
    w_val[rng.random((V, 4)) < np.array([0, 0.2, 0.6, 0.8])] = 0.0
    for c in range(1, 4):                                       # one entry per bone: a repeated bone keeps its first entry
        dup = (w_idx[:, c:c + 1] == w_idx[:, :c]).any(1)
        w_val[dup, c] = 0.0
    w_val /= w_val.sum(1, keepdims=True)
    # exact duplicates (equal distances to every query), some of them three times
    src = np.array([100, 101, 102, 103, 104, 2500, 2501, 6000])
    verts[3000:3008] = verts[src]
    verts[6880:6883] = verts[src[:3]]
    return verts, w_idx, w_val.astype(np.float32)


def dense_weights(w_idx, w_val):
    W = np.zeros((w_idx.shape[0], 24), np.float32)
    for c in range(w_idx.shape[1]):
        np.add.at(W, (np.arange(W.shape[0]), w_idx[:, c].astype(np.int64)), w_val[:, c])
    return W


def run_reference(dt, verts, W, resolution, sweeps_at=()):
    """switch_to_explicit(use_smpl=True) at `resolution` with the intermediate stages recorded."""
    rec = {}
    real_knn = sys.modules["lib.pytorch3d.ops"].knn_points
    real_q = dt.query_weights_smpl

    def knn_rec(*a, **kw):
        if "_out" in rec:                                       # the second call of a run (inside the reference's function): same arguments
            return rec["_out"]
        out = rec["_out"] = real_knn(*a, **kw)
        rec["d2"], rec["idx"] = out.dists[0].numpy().copy(), out.idx[0].numpy().copy()
        return out

    def query_rec(x, smpl_verts, smpl_weights, resolution=128):
        rec["grid_points"] = x[0].numpy().copy()
        # the body of query_weights_smpl up to the reshape, evaluated by the reference's own expressions
        dist, idx, _ = dt.ops.knn_points(x, smpl_verts.detach(), K=K)
        dist = dist.sqrt().clamp_(0.0001, 1.)
        weights = smpl_weights[0, idx]
        ws = 1. / dist
        ws = ws / ws.sum(-1, keepdim=True)
        rec["blend"] = (ws[..., None] * weights).sum(-2)[0].T.contiguous().numpy().copy()      # [24, P]
        return real_q(x, smpl_verts, smpl_weights, resolution=resolution)

    dt.ops.knn_points = knn_rec
    dt.query_weights_smpl = query_rec
    real_lin = torch.linspace
    torch.linspace = scalar_linspace
    try:
        d = dt.ForwardDeformer.__new__(dt.ForwardDeformer)
        torch.nn.Module.__init__(d)
        d.global_scale = 1.2
        d.device = "cpu"
        d.switch_to_explicit(resolution=resolution, smpl_verts=torch.from_numpy(verts)[None], smpl_weights=torch.from_numpy(W)[None],
                             use_smpl=True)
    finally:
        torch.linspace = real_lin
        dt.ops.knn_points = real_knn
        dt.query_weights_smpl = real_q
    del rec["_out"]
    rec.update(lbs_voxel_final=d.lbs_voxel_final.numpy(), offset=d.offset.numpy().reshape(3), scale=np.float32(d.scale.item()),
               offset_kernel=d.offset_kernel.numpy().reshape(3), scale_kernel=d.scale_kernel.numpy().reshape(3), bbox=d.bbox.numpy())
    return rec


def sweeps(w, n):
    """n sweeps of deformer_torch.py:246-252 on [1,24,D,H,W] (the reference's lines, to record the grid after one sweep)."""
    weights = w.clone()
    for _ in range(n):
        mean = (weights[:, :, 2:, 1:-1, 1:-1] + weights[:, :, :-2, 1:-1, 1:-1] + weights[:, :, 1:-1, 2:, 1:-1]
                + weights[:, :, 1:-1, :-2, 1:-1] + weights[:, :, 1:-1, 1:-1, 2:] + weights[:, :, 1:-1, 1:-1, :-2]) / 6.0
        weights[:, :, 1:-1, 1:-1, 1:-1] = (weights[:, :, 1:-1, 1:-1, 1:-1] - mean) * 0.7 + mean
        sums = weights.sum(1, keepdim=True)
        weights = weights / sums
    return weights


def main():
    tmp = tempfile.mkdtemp(prefix="golden_skinning_")
    knn_ext = build_knn_cpu(tmp)
    dt, sd = load_reference(knn_ext)
    verts, w_idx, w_val = make_body()
    W = dense_weights(w_idx, w_val)
    ops = sys.modules["lib.pytorch3d.ops"]

    r32 = run_reference(dt, verts, W, 32)
    # the reference's own layout: a [1,P,24] tensor seen as [1,24,D,H,W] (channel stride 1), which decides torch's order in sum(1)
    w0 = torch.from_numpy(np.ascontiguousarray(r32["blend"].T))[None].permute(0, 2, 1).reshape(1, 24, 8, 32, 32)
    after1 = sweeps(w0, 1).numpy()[0]
    after30 = sweeps(w0, 30).numpy()[0]
    assert np.array_equal(after30, r32["lbs_voxel_final"][0])            # the recorded blend is what the reference smoothed
    # ties: some query has two duplicated vertices among its K, in index order
    dup_pairs = sum(int(((r32["idx"] == a).any(1) & (r32["idx"] == b).any(1)).sum()) for a, b in ((100, 3000), (101, 3001), (2500, 3005)))
    assert dup_pairs > 0

    r128 = run_reference(dt, verts, W, 128)
    sel = np.arange(0, 32 * 128 * 128, 1021)
    lin_diffs = {n: int((scalar_linspace(-1, 1, n).numpy().view(np.uint32) != torch.linspace(-1, 1, n).numpy().view(np.uint32)).sum())
                 for n in (8, 32, 128)}

    small = {}
    rng = np.random.default_rng(5)
    for tag, (P, Vs, Ks) in {"a": (1, 32, 32), "b": (300, 777, 1), "c": (257, 1543, 32), "d": (64, 33, 7)}.items():
        p1 = rng.normal(size=(P, 3)).astype(np.float32)
        p2 = rng.normal(size=(Vs, 3)).astype(np.float32)
        p2[Vs // 2:Vs // 2 + 3] = p2[:3]                                  # ties
        p2 = np.round(p2 * 8) / 8 if tag == "c" else p2                    # a coarse lattice: many equal distances
        p1 = np.round(p1 * 8) / 8 if tag == "c" else p1
        out = ops.knn_points(torch.from_numpy(p1)[None], torch.from_numpy(p2)[None], K=Ks)
        small.update({f"small_{tag}_p1": p1, f"small_{tag}_p2": p2.astype(np.float32), f"small_{tag}_K": np.int32(Ks),
                      f"small_{tag}_d2": out.dists[0].numpy(), f"small_{tag}_idx": out.idx[0].numpy().astype(np.int16)})

    vs = torch.from_numpy(verts)[None]
    smpl = {"bbox_from_vertices": sd.get_bbox_from_smpl(vs).numpy(), "bbox_from_vertices_15": sd.get_bbox_from_smpl(vs, factor=1.5).numpy(),
            "rest_pose_da_pose": sd.get_predefined_rest_pose("da_pose", device="cpu").numpy(),
            "rest_pose_a_pose": sd.get_predefined_rest_pose("A_pose", device="cpu").numpy()}

    np.savez_compressed(os.path.join(HERE, "golden_skinning.npz"), verts=verts, w_idx=w_idx, w_val=w_val,
                        offset=r32["offset"], scale=r32["scale"], offset_kernel=r32["offset_kernel"], scale_kernel=r32["scale_kernel"],
                        bbox=r32["bbox"], grid_points_32=r32["grid_points"], idx_32=r32["idx"].astype(np.int16),
                        sel_128=sel.astype(np.int32), grid_points_128=r128["grid_points"][sel], idx_128=r128["idx"][sel].astype(np.int16),
                        d2_128=r128["d2"][sel], blend_128=r128["blend"][:, sel], final_128=r128["lbs_voxel_final"][0].reshape(24, -1)[:, sel],
                        linspace_host_diffs=np.array([lin_diffs[8], lin_diffs[32], lin_diffs[128]]), **small, **smpl)
    np.savez_compressed(os.path.join(HERE, "golden_skinning_d2.npz"), d2_32=r32["d2"])
    np.savez_compressed(os.path.join(HERE, "golden_skinning_blend.npz"), blend_32=r32["blend"], after1_32=after1)
    np.savez_compressed(os.path.join(HERE, "golden_skinning_grid.npz"), after30_32=after30)
    for f in ("", "_d2", "_blend", "_grid"):
        p = os.path.join(HERE, f"golden_skinning{f}.npz")
        print(p, os.path.getsize(p))
        assert os.path.getsize(p) < (1 << 20), p
    print("duplicate pairs inside one K list:", dup_pairs, "linspace host diffs:", lin_diffs)


if __name__ == "__main__":
    main()
