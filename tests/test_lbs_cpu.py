"""Forward skinning and vertex normals without a GPU: intrinsicavatar_amd/csrc/lbs_math.h replayed on the host by tests/lbs_harness.c
against tests/golden/golden_lbs*.npz (the reference's own query_weights closure and skinning_mask on the CPU,
tests/golden/make_golden_lbs.py) and against an fp64 numpy accumulation of the normals; the OBJ / npz writers.

Bars (tests/golden/lbs_parity_bars.json, written by tools/lbs_parity_probe.py): 3 x the observed maximum, under hard ceilings that do
not come from the code under test --
    w      1e-5 absolute: a weight is a convex combination (8 corners) of values in [0, 1]; 24 fp32 terms cannot lose more
    R      1e-5 x max |tfs|: an entry of R is a convex combination of 24 entries of tfs (the same reasoning, scaled)
    xd     1e-5 x max |tfs| x the box's longest side
    normal 1e-5 absolute on unit vectors: a vertex of the fixture mesh sums at most 13 face vectors that do not cancel (a convex
           surface), each a few roundings of 6e-8 relative
The reference normalises with (x - offset) / scale [* ratio], the kernel with (x + offset_kernel) * scale_kernel as the search kernels
do; the two differ by roundings of the coordinate, which the bars cover."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
W_CEIL = 1e-5
NRM_CEIL = 1e-5

vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)      # noqa: E731


def build_harness(directory):
    so = os.path.join(str(directory), "liblbs_harness.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-fvisibility=hidden", "-o", so,
                           os.path.join(HERE, "lbs_harness.c"), "-lm"])
    return C.CDLL(so)


def load_golden():
    g = {}
    for f in ("golden_lbs.npz", "golden_lbs_w.npz"):
        z = np.load(os.path.join(GOLDEN, f))
        g.update({k: z[k] for k in z.files})
    g["mesh_f"] = g["mesh_f"].astype(np.int64)
    return g


def bars():
    return json.load(open(os.path.join(GOLDEN, "lbs_parity_bars.json")))


def ceilings(g):
    """hard ceilings of the module docstring for this fixture: {"w", "R", "xd", "normal"}"""
    tmax = float(np.abs(g["tfs"]).max())
    side = float((g["bbox"][1] - g["bbox"][0]).max())
    return {"w": W_CEIL, "R": 1e-5 * tmax, "xd": 1e-5 * tmax * side, "normal": NRM_CEIL}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def h_forward(h, g, xc, want=("w", "xd", "R"), tfs="fixture"):
    xc = np.ascontiguousarray(xc, np.float32).reshape(-1, 3)
    P = xc.shape[0]
    grid = np.ascontiguousarray(g["grid"], np.float32)
    _, _, D, H, W = grid.shape
    tfs = np.ascontiguousarray(g["tfs"] if isinstance(tfs, str) else tfs, np.float32)
    out = {"w": np.zeros((P, 24), np.float32) if "w" in want else None, "xd": np.zeros((P, 3), np.float32) if "xd" in want else None,
           "R": np.zeros((P, 3, 3), np.float32) if "R" in want else None}
    off, sc = np.ascontiguousarray(g["offset_kernel"], np.float32), np.ascontiguousarray(g["scale_kernel"], np.float32)
    h.lbs_h_forward(C.c_int64(P), vp(xc), vp(grid), C.c_int(D), C.c_int(H), C.c_int(W), vp(off), vp(sc), vp(tfs), vp(out["w"]),
                    vp(out["xd"]), vp(out["R"]))
    return out


def h_corners(h, g, xc):
    xc = np.ascontiguousarray(xc, np.float32).reshape(-1, 3)
    _, _, D, H, W = g["grid"].shape
    cell = np.zeros((xc.shape[0], 3), np.int32)
    mask = np.zeros(xc.shape[0], np.int32)
    off, sc = np.ascontiguousarray(g["offset_kernel"], np.float32), np.ascontiguousarray(g["scale_kernel"], np.float32)
    h.lbs_h_corners(C.c_int64(xc.shape[0]), vp(xc), C.c_int(D), C.c_int(H), C.c_int(W), vp(off), vp(sc), vp(cell), vp(mask))
    return cell, mask


def h_normals(h, v, f):
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int64)
    offsets = np.zeros(len(v) + 1, np.int32)
    lists = np.zeros(max(3 * len(f), 1), np.int32)
    nrm = np.zeros((len(v), 3), np.float32)
    assert h.lbs_h_vertex_normals(C.c_int64(len(v)), C.c_int64(len(f)), vp(v), vp(f), vp(offsets), vp(lists), vp(nrm)) == 0
    return nrm, offsets, lists[:3 * len(f)]


def normals_fp64(v, f):
    """the definition in fp64 numpy: np.add.at of the un-normalised face cross products, then n / max(|n|, 1e-12)"""
    p = np.asarray(v, np.float64)
    c = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    n = np.zeros_like(p)
    for k in range(3):
        np.add.at(n, f[:, k], c)
    return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-12)


def rigid_transform(seed=3):
    """one rigid 4 x 4 (float32): a rotation by 0.9 rad about a seeded axis, and a translation"""
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    A = np.eye(4)
    A[:3, :3] = np.eye(3) + np.sin(0.9) * K + (1 - np.cos(0.9)) * (K @ K)
    A[:3, 3] = rng.normal(size=3) * 0.3
    return A.astype(np.float32)


def mesh_in_box(g):
    """the fixture mesh scaled into the grid's box: (v_pos float32 [V,3], t_pos_idx int64 [T,3])"""
    lo, hi = g["bbox"][0].astype(np.float64), g["bbox"][1].astype(np.float64)
    v = (lo + hi) / 2 + g["mesh_v"].astype(np.float64) * (hi - lo) / 2 * 0.95
    return v.astype(np.float32), g["mesh_f"]


def permuted_faces(f):
    return np.ascontiguousarray(f[np.random.default_rng(1).permutation(len(f))])


def measure_host(h, g):
    """{name: max abs difference} of the host replay: to the reference fixture (w, xd, R) and to the fp64 normals"""
    out = h_forward(h, g, g["xc"])
    m = {k: float(np.abs(out[k].astype(np.float64) - g[k]).max()) for k in ("w", "xd", "R")}
    nrm, _, _ = h_normals(h, g["mesh_v"], g["mesh_f"])
    m["normal"] = float(np.abs(nrm.astype(np.float64) - normals_fp64(g["mesh_v"], g["mesh_f"])).max())
    return m


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("lbs"))


@pytest.fixture(scope="module")
def g():
    return load_golden()


def test_fixture_is_what_the_issue_asks_for(g):
    assert g["grid"].shape == (1, 24, 4, 16, 16) and g["xc"].shape == (4096, 3) and g["w"].shape == (4096, 24)
    assert (g["grid"] > 0).all() and np.abs(g["grid"].sum(1) - 1).max() < 1e-6
    assert abs(g["scale_kernel"][2] / g["scale_kernel"][0] - 4.0) < 1e-6 and np.abs(g["offset_kernel"]).min() > 1e-3
    assert [int((g["kind"] == k).sum()) for k in range(5)] == [2570, 600, 300, 600, 26]
    # rigid transforms
    R = g["tfs"][:, :3, :3].astype(np.float64)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6 and np.abs(np.linalg.det(R) - 1).max() < 1e-6
    gn = (g["xc"] + g["offset_kernel"]) * g["scale_kernel"]
    assert (np.abs(gn[g["kind"] == 0]) < 1).all() and (np.abs(gn[g["kind"] >= 3]).max(1) > 1).all()
    regions = {tuple(np.sign(r) * (np.abs(r) > 1)) for r in gn[g["kind"] == 4]}
    assert len(regions) == 26                                        # every face, edge and corner region outside the box
    for a in range(3):                                               # both sides of every axis
        assert (gn[g["kind"] == 3][:, a] > 1).any() and (gn[g["kind"] == 3][:, a] < -1).any()


def test_replay_reproduces_the_reference(harness, g):
    m = measure_host(harness, g)
    print("host replay vs fixture (max abs):", m)
    rec, ceil = bars()["host_replay"], ceilings(g)
    for k in ("w", "xd", "R"):
        assert m[k] <= ceil[k], (k, m[k], ceil[k])
        assert m[k] <= 3 * rec[k], (k, m[k], rec[k])                 # the recorded observation still describes the code
    out = h_forward(harness, g, g["xc"])
    assert np.abs(out["w"].sum(1) - 1).max() < 1e-5


def test_each_nullable_combination_gives_the_same_bits(harness, g):
    xc = g["xc"][::16]
    full = h_forward(harness, g, xc)
    for want in (("w",), ("xd",), ("R",), ("w", "xd"), ("w", "R"), ("xd", "R")):
        part = h_forward(harness, g, xc, want)
        for k in ("w", "xd", "R"):
            assert (part[k] is None) == (k not in want)
            if k in want:
                assert np.array_equal(bits(part[k]), bits(full[k])), (want, k)


def test_corners_that_carry_weight(harness, g):
    """discrete facts, no tolerance: the cell and which of its corners are inside, against a float32 numpy restatement"""
    cell, mask = h_corners(harness, g, g["xc"])
    f32 = np.float32
    gn = ((g["xc"] + g["offset_kernel"]).astype(f32) * g["scale_kernel"]).astype(f32)
    _, _, D, H, W = g["grid"].shape
    want_cell, inside = [], []
    for a, n in enumerate((W, H, D)):
        idx = (((gn[:, a] + f32(1)) / f32(2)).astype(f32) * f32(n - 1)).astype(f32)
        idx = np.minimum(np.maximum(idx, f32(0)), f32(n - 1))
        c0 = np.floor(idx).astype(np.int32)
        want_cell.append(c0)
        inside.append(c0 + 1 < n)
    assert np.array_equal(cell, np.stack(want_cell, 1))
    want_mask = np.zeros(len(gn), np.int32)
    for k in range(8):
        ok = np.ones(len(gn), bool)
        for a in range(3):
            if (k >> a) & 1:
                ok &= inside[a]
        want_mask |= ok.astype(np.int32) << k
    assert np.array_equal(mask, want_mask)
    # points on the last node of an axis (to a rounding: some land an ulp inside it), or past it, load no corner beyond it
    assert (mask[g["kind"] == 2] != 0xFF).any() and (mask[(gn > 1).any(1)] != 0xFF).all() and (mask[(gn > 1).all(1)] == 1).all()
    assert (mask[(gn < 1).all(1)] == 0xFF).all()


def test_out_of_box_points_sample_the_border(harness, g):
    out = g["kind"] >= 3
    gn = (g["xc"][out] + g["offset_kernel"]) * g["scale_kernel"]
    clamped = (np.clip(gn, -1, 1) / g["scale_kernel"] - g["offset_kernel"]).astype(np.float32)
    a, b = h_forward(harness, g, g["xc"][out], ("w",))["w"], h_forward(harness, g, clamped, ("w",))["w"]
    # the clamped point is rebuilt through a division: its index moves by roundings, (n - 1) x 2^-22 per axis at the most
    _, _, D, H, W = g["grid"].shape
    assert np.abs(a - b).max() <= (D + H + W - 3) * 2.0 ** -22


def test_normals_equal_the_fp64_accumulation(harness, g):
    v, f = g["mesh_v"], g["mesh_f"]
    nrm, offsets, lists = h_normals(harness, v, f)
    want = normals_fp64(v, f)
    err = float(np.abs(nrm.astype(np.float64) - want).max())
    print("normals vs fp64 (max abs):", err)
    assert err <= NRM_CEIL and err <= 3 * bars()["host_replay"]["normal"]
    # the fixture mesh: closed sphere + a vertex of valence >= 12 + a zero-area face
    valence = np.diff(offsets)
    assert valence.max() >= 12 and offsets[-1] == 3 * len(f) and (valence > 0).all()
    area2 = np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    assert (area2 == 0).sum() == 1
    ns = int(g["mesh_n_sphere"])
    sphere_f = f[(f < ns).all(1) & (area2 > 0)]
    e = np.sort(np.concatenate([sphere_f[:, [0, 1]], sphere_f[:, [1, 2]], sphere_f[:, [2, 0]]]), axis=1)
    assert (np.unique(e, axis=0, return_counts=True)[1] == 2).all()          # closed
    assert ((nrm[:ns] * v[:ns]).sum(1) > 0).all()                            # outward
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1).max() < 1e-6
    # the lists: every vertex's faces, ascending
    for vtx in range(len(v)):
        mine = lists[offsets[vtx]:offsets[vtx + 1]]
        assert np.array_equal(mine, np.sort(np.concatenate([np.nonzero(f[:, k] == vtx)[0] for k in range(3)])))


def test_normals_ignore_bad_faces_and_isolated_vertices(harness):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 4], [-1, 1, 2]], np.int64)
    nrm, offsets, _ = h_normals(harness, v, f)
    assert offsets.tolist() == [0, 1, 2, 3, 3]
    assert np.array_equal(nrm, np.array([[0, 0, 1]] * 3 + [[0, 0, 0]], np.float32))


def test_harness_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lbs_harness")
    subprocess.check_call(["gcc", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DLBS_HARNESS_MAIN", "-o", exe, os.path.join(HERE, "lbs_harness.c"), "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "lbs_harness OK" in out.stdout, out.stdout[-1000:] + out.stderr[-3000:]


OBJ_PLAIN = "v 0 0 0\nv 1 0 0.5\nv 0.100000001 -2 3\nf 1 2 3\nf 3 2 1\n"


def test_save_obj_without_normals_is_unchanged_and_with_normals_round_trips(tmp_path):
    from intrinsicavatar_amd import io_formats
    v = np.array([[0, 0, 0], [1, 0, 0.5], [0.1, -2, 3]], np.float32)
    f = np.array([[0, 1, 2], [2, 1, 0]], np.int64)
    p = str(tmp_path / "a.obj")
    io_formats.save_obj(p, v, f)
    assert open(p).read() == OBJ_PLAIN
    io_formats.save_obj(p, v, f, None)
    assert open(p).read() == OBJ_PLAIN
    n = np.array([[0, 0, 1], [0.6, 0, -0.8], [0.26726124, 0.53452248, 0.80178373]], np.float32)
    io_formats.save_obj(p, v, f, n)
    text = open(p).read()
    assert text.count("\nvn ") == 3 and "f 1//1 2//2 3//3\n" in text and text.startswith("v 0 0 0\n")
    v2, f2, n2 = io_formats.load_obj(p, with_normals=True)
    assert np.array_equal(bits(v2), bits(v)) and np.array_equal(f2, f) and np.array_equal(bits(n2), bits(n))
    v3, f3 = io_formats.load_obj(p)
    assert np.array_equal(bits(v3), bits(v)) and np.array_equal(f3, f)
    with pytest.raises(ValueError):
        io_formats.save_obj(p, v, f, n[:2])


def test_save_skinned_npz(tmp_path, g):
    from intrinsicavatar_amd import io_formats
    v, f = g["mesh_v"], g["mesh_f"]
    rng = np.random.default_rng(0)
    w = rng.random((len(v), 24)).astype(np.float32)
    mesh = {"v_pos": v, "t_pos_idx": f, "v_nrm": normals_fp64(v, f).astype(np.float32)}
    p = str(tmp_path / "sub" / "m.npz")
    io_formats.save_skinned_npz(p, mesh, w, g["tfs"])
    z = np.load(p)
    assert sorted(z.files) == ["t_pos_idx", "tfs", "v_nrm", "v_pos", "weights"]
    assert np.array_equal(z["v_pos"], v) and np.array_equal(z["t_pos_idx"], f) and np.array_equal(z["weights"], w)
    assert z["v_nrm"].dtype == np.float32 and z["tfs"].shape == (24, 4, 4)
    io_formats.save_skinned_npz(p, mesh, w)
    assert "tfs" not in np.load(p).files
    with pytest.raises(ValueError):
        io_formats.save_skinned_npz(p, mesh, w[:, :23])
    with pytest.raises(ValueError):
        io_formats.save_skinned_npz(p, {"v_pos": v, "t_pos_idx": f}, w)


def test_no_cpu_fallback_and_cli_argument_checks(g):
    import torch
    from intrinsicavatar_amd import _lib, fast_snarf, mesh
    from intrinsicavatar_amd.deformer import SNARFDeformer
    T = torch.from_numpy
    with pytest.raises(_lib.IaError):
        mesh.vertex_normals(T(g["mesh_v"]), T(g["mesh_f"]))
    with pytest.raises(_lib.IaError):
        fast_snarf.forward_skinning(T(g["xc"]), T(g["grid"]), T(g["tfs"]), T(g["offset_kernel"]), T(g["scale_kernel"]))
    assert SNARFDeformer.forward_skinning.__doc__ and callable(fast_snarf.forward_skinning)
    with pytest.raises(SystemExit):
        mesh.main(["--state-dict", "x", "--out", "y", "--bbox", "0", "0", "0", "1", "1", "1", "--pose-npz", "p.npz"])       # needs --smpl-npz
    with pytest.raises(SystemExit):
        mesh.main(["--state-dict", "x", "--out", "y", "--bbox", "0", "0", "0", "1", "1", "1", "--skinned-npz", "s.npz"])   # needs --pose-npz
