"""Forward skinning (csrc/lbs_fwd.hip), vertex normals (csrc/mesh_attr.hip) and mesh.pose on the MI355X, against
tests/golden/golden_lbs*.npz (the reference's own query_weights closure + skinning_mask), the fp64 numpy normals, and the host replay
of the same arithmetic (tests/lbs_harness.c).  Bars: tests/golden/lbs_parity_bars.json "gpu" = 3 x the MI355X observation
(tools/lbs_parity_probe.py), under the hard ceilings stated in tests/test_lbs_cpu.py; discrete facts -- face lists, offsets, which
corners carry weight (the host replay's, bit for bit) -- have no tolerance."""
import itertools

import numpy as np
import pytest
import torch

from tests.test_lbs_cpu import (bars, bits, build_harness, ceilings, h_forward, h_normals, load_golden, mesh_in_box, normals_fp64,
                                permuted_faces, rigid_transform)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("lbs_gpu"))


@pytest.fixture(scope="module")
def g():
    return load_golden()


@pytest.fixture(scope="module")
def dfm(g):
    from intrinsicavatar_amd.deformer import SNARFDeformer
    d = SNARFDeformer(T(g["grid"]), T(g["offset_kernel"]), T(g["scale_kernel"]), T(g["bbox"]))
    d.tfs = T(g["tfs"])[None]
    return d


@pytest.fixture(scope="module")
def full(g):
    """the kernel's three outputs on the fixture's points, computed once: {"xd", "R", "w"} (device tensors, never written)"""
    from intrinsicavatar_amd import fast_snarf
    xd, R, w = fast_snarf.forward_skinning(T(g["xc"]), T(g["grid"]), T(g["tfs"]), T(g["offset_kernel"]), T(g["scale_kernel"]),
                                           want_weights=True)
    return {"xd": xd, "R": R, "w": w}


def held(name, got, want, ceil):
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())
    bar = bars()["gpu"][name]
    print(f"{name}: max abs difference {err:.3e} (bar {bar:.3e}, ceiling {ceil:.3e})")
    assert err <= ceil, (name, err, ceil)
    assert err <= bar, (name, err, bar)


def normal_error_bound(p, fn):
    """per-vertex a-priori bound on |fp32 normal - fp64 normal| for any mesh: a face vector computed in fp32 is off by at most
    ~4 x 2^-24 |e1| |e2| (two products and a difference per component, edge differences of float32 inputs), a vertex sums its faces'
    errors and a few roundings of the sum, and the direction of the sum moves by that over its length; 1e-6 for the normalisation"""
    e1, e2 = p[fn[:, 1]] - p[fn[:, 0]], p[fn[:, 2]] - p[fn[:, 0]]
    prod = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)
    tot, raw = np.zeros(len(p)), np.zeros_like(p)
    for k in range(3):
        np.add.at(tot, fn[:, k], prod)
        np.add.at(raw, fn[:, k], np.cross(e1, e2))
    return 8 * 2.0 ** -24 * tot / np.linalg.norm(raw, axis=1) + 1e-6


def test_forward_skinning_matches_the_reference(g, full):
    ceil = ceilings(g)
    for k in ("w", "xd", "R"):
        assert full[k].shape == g[k].shape and full[k].dtype == torch.float32
        held(k, full[k].cpu().numpy(), g[k], ceil[k])
    assert float((full["w"].sum(1) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("want", [c for n in (1, 2) for c in itertools.combinations(("w", "xd", "R"), n)], ids="+".join)
def test_each_nullable_combination(g, full, want):
    from intrinsicavatar_amd import fast_snarf
    tfs = T(g["tfs"]) if ("xd" in want or "R" in want) else None           # the weights alone need no transforms
    xd, R, w = fast_snarf.forward_skinning(T(g["xc"]), T(g["grid"]), tfs, T(g["offset_kernel"]), T(g["scale_kernel"]),
                                           want_weights="w" in want, want_xd="xd" in want, want_rot="R" in want)
    got = {"xd": xd, "R": R, "w": w}
    ceil = ceilings(g)
    for k in ("w", "xd", "R"):
        assert (got[k] is None) == (k not in want)
        if k in want:
            held(k, got[k].cpu().numpy(), g[k], ceil[k])
            assert torch.equal(got[k], full[k]), (want, k)


def test_kernel_equals_the_host_replay_bit_for_bit(harness, g, full):
    """the same expressions, compiled by gcc and by hipcc without contraction: every output word, hence also which corners carried
    weight"""
    ref = h_forward(harness, g, g["xc"])
    for k in ("w", "xd", "R"):
        assert np.array_equal(bits(full[k].cpu().numpy()), bits(ref[k])), k


def test_deformer_methods_are_the_kernel(g, dfm, full):
    assert torch.equal(dfm.query_weights(T(g["xc"])), full["w"])
    xd, R = dfm.forward_skinning(T(g["xc"]))
    assert torch.equal(xd, full["xd"]) and torch.equal(R, full["R"])
    xd, R, w = dfm.forward_skinning(T(g["xc"]), want_weights=True, want_rot=False)
    assert R is None and torch.equal(xd, full["xd"]) and torch.equal(w, full["w"])
    # any leading shape, as the reference's closure takes it
    assert torch.equal(dfm.query_weights(T(g["xc"]).reshape(64, 64, 3)), full["w"])


def test_out_of_box_points_equal_their_clamped_points(g, full):
    """the box in the kernel's own coordinates g = (x + offset) * scale in [-1, 1]: every outside coordinate is moved onto the box
    face -- to the float32 nearest the face whose g is still >= 1 (<= -1) -- and the weights must not change by a bit"""
    from intrinsicavatar_amd import fast_snarf
    f32 = np.float32
    sel = g["kind"] >= 3
    x = g["xc"][sel].copy()
    off, sc = g["offset_kernel"].astype(f32), g["scale_kernel"].astype(f32)
    gn = ((x + off).astype(f32) * sc).astype(f32)
    hi, lo = gn > 1, gn < -1
    assert hi.any(0).all() and lo.any(0).all()
    face_hi = (1.0 / sc.astype(np.float64) - off).astype(f32)
    face_lo = (-1.0 / sc.astype(np.float64) - off).astype(f32)
    c = np.where(hi, face_hi[None], np.where(lo, face_lo[None], x)).astype(f32)
    for _ in range(4):                                     # a rounding may leave the face an ulp inside: step outward
        gc = ((c + off).astype(f32) * sc).astype(f32)
        c = np.where(hi & (gc < 1), np.nextafter(c, f32(np.inf)), np.where(lo & (gc > -1), np.nextafter(c, f32(-np.inf)), c)).astype(f32)
    gc = ((c + off).astype(f32) * sc).astype(f32)
    assert (gc[hi] >= 1).all() and (gc[lo] <= -1).all() and np.abs(gc[hi] - 1).max() < 1e-6 and np.abs(gc[lo] + 1).max() < 1e-6
    _, _, w = fast_snarf.forward_skinning(T(c), T(g["grid"]), None, T(g["offset_kernel"]), T(g["scale_kernel"]), want_weights=True,
                                          want_xd=False, want_rot=False)
    assert torch.equal(w, full["w"][T(np.nonzero(sel)[0])])


@pytest.mark.parametrize("P", [1, 63, 65, 4096])
def test_a_point_does_not_depend_on_its_launch(g, full, P):
    from intrinsicavatar_amd import fast_snarf
    xd, R, w = fast_snarf.forward_skinning(T(g["xc"][:P]), T(g["grid"]), T(g["tfs"]), T(g["offset_kernel"]), T(g["scale_kernel"]),
                                           want_weights=True)
    assert w.shape == (P, 24) and xd.shape == (P, 3) and R.shape == (P, 3, 3)
    assert torch.equal(w[0], full["w"][0]) and torch.equal(xd[0], full["xd"][0]) and torch.equal(R[0], full["R"][0])
    assert torch.equal(w, full["w"][:P]) and torch.equal(xd, full["xd"][:P])


def test_vertex_normals_on_the_fixture_mesh(harness, g):
    from intrinsicavatar_amd import mesh
    v, f = g["mesh_v"], g["mesh_f"]
    nrm, offsets, lists = mesh.vertex_normals(T(v), T(f), return_lists=True)
    assert nrm.shape == (len(v), 3) and nrm.dtype == torch.float32
    held("normal", nrm.cpu().numpy(), normals_fp64(v, f), ceilings(g)["normal"])
    # discrete facts and the host replay: no tolerance
    h_nrm, h_off, h_lists = h_normals(harness, v, f)
    assert np.array_equal(offsets.cpu().numpy(), h_off) and np.array_equal(lists.cpu().numpy(), h_lists)
    assert np.array_equal(bits(nrm.cpu().numpy()), bits(h_nrm))
    # two runs
    assert torch.equal(mesh.vertex_normals(T(v), T(f)), nrm)
    ns = int(g["mesh_n_sphere"])
    assert bool(((nrm[:ns] * T(v)[:ns]).sum(1) > 0).all())


def test_vertex_normals_of_a_permuted_face_array(harness, g):
    """the per-vertex sort fixes the summation order up to the relabelling of the faces: the device equals the host replay of the
    permuted mesh bit for bit, and the un-permuted normals within the fp64 bar"""
    from intrinsicavatar_amd import mesh
    v, f = g["mesh_v"], g["mesh_f"]
    fp = permuted_faces(f)
    nrm, offsets, lists = mesh.vertex_normals(T(v), T(fp), return_lists=True)
    h_nrm, h_off, h_lists = h_normals(harness, v, fp)
    assert np.array_equal(bits(nrm.cpu().numpy()), bits(h_nrm))
    assert np.array_equal(offsets.cpu().numpy(), h_off) and np.array_equal(lists.cpu().numpy(), h_lists)
    held("normal_permuted", nrm.cpu().numpy(), normals_fp64(v, f), ceilings(g)["normal"])


def test_vertex_normals_of_a_mesh_of_many_blocks(harness, g):
    """a marching-cubes sphere at 40^3 (thousands of vertices: many workgroups, lists filled by concurrent atomics) + faces with bad
    indices"""
    from intrinsicavatar_amd import mesh
    ax = torch.linspace(-1, 1, 40, device=DEV)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    m = mesh.marching_cubes((X * X + Y * Y + Z * Z).sqrt() - 0.7, 0.0, (-1, -1, -1), (1, 1, 1))
    v, f = m["v_pos"], m["t_pos_idx"]
    assert v.shape[0] > 2000
    bad = torch.tensor([[0, 1, v.shape[0]], [-1, 2, 3]], dtype=torch.int64, device=DEV)
    f2 = torch.cat([f[:100], bad, f[100:]])
    nrm, offsets, lists = mesh.vertex_normals(v, f2, return_lists=True)
    assert int(offsets[-1]) == 3 * f.shape[0]
    h_nrm, h_off, h_lists = h_normals(harness, v.cpu().numpy(), f2.cpu().numpy())
    n_listed = int(h_off[-1])
    assert np.array_equal(offsets.cpu().numpy(), h_off) and np.array_equal(lists.cpu().numpy()[:n_listed], h_lists[:n_listed])
    assert np.array_equal(bits(nrm.cpu().numpy()), bits(h_nrm))
    assert torch.equal(mesh.vertex_normals(v, f2), nrm)
    p, fn = v.cpu().numpy().astype(np.float64), f.cpu().numpy()
    bound = normal_error_bound(p, fn)
    err = np.abs(nrm.cpu().numpy() - normals_fp64(p, fn)).max(1)
    print("40^3 sphere: max normal error", float(err.max()), "largest bound", float(bound.max()))
    assert (err <= bound).all()
    assert bool(((nrm * v).sum(1) > 0).all())
    # no faces at all: zero normals
    none = mesh.vertex_normals(v[:10], f[:0])
    assert none.shape == (10, 3) and float(none.abs().max()) == 0.0


def test_pose_with_identity_transforms(g, dfm):
    from intrinsicavatar_amd import mesh
    v, f = mesh_in_box(g)
    cano = {"v_pos": T(v), "t_pos_idx": T(f)}
    tfs0 = dfm.tfs
    try:
        dfm.tfs = torch.eye(4, device=DEV).expand(1, 24, 4, 4).contiguous()
        posed = mesh.pose(cano, dfm)
    finally:
        dfm.tfs = tfs0
    assert sorted(posed) == ["t_pos_idx", "v_nrm", "v_pos"] and posed["t_pos_idx"] is cano["t_pos_idx"]
    side = float((g["bbox"][1] - g["bbox"][0]).max())
    held("pose_identity_xd", posed["v_pos"].cpu().numpy(), v, 1e-5 * 1.0 * side)
    # the normals are the canonical definition evaluated on the posed vertices, bit for bit
    assert torch.equal(posed["v_nrm"], mesh.vertex_normals(posed["v_pos"], cano["t_pos_idx"]))
    held("pose_identity_normal", posed["v_nrm"].cpu().numpy(), normals_fp64(posed["v_pos"].cpu().numpy(), f), ceilings(g)["normal"])
    w = mesh.skinning_weights(cano, dfm)
    assert w.shape == (len(v), 24) and torch.equal(w, dfm.query_weights(cano["v_pos"]))


def test_pose_with_one_rigid_transform_on_all_bones(g, dfm):
    """xd = A v and the normals are the rotated canonical normals.  Ceilings: xd as in forward skinning; a posed vertex carries at most
    ~4 roundings of 2^-24 |v|, an edge vector twice that, so the direction of a face vector (and of their sum) moves by at most
    16 x 2^-24 x max |v| / the shortest edge, on top of the normals' own ceiling."""
    from intrinsicavatar_amd import mesh
    v, f = mesh_in_box(g)
    A = rigid_transform().astype(np.float64)
    cano = {"v_pos": T(v), "t_pos_idx": T(f)}
    tfs0 = dfm.tfs
    try:
        dfm.tfs = T(A.astype(np.float32))[None, None].expand(1, 24, 4, 4).contiguous()
        posed = mesh.pose(cano, dfm)
    finally:
        dfm.tfs = tfs0
    want_v = v.astype(np.float64) @ A[:3, :3].T + A[:3, 3]
    want_n = normals_fp64(v, f) @ A[:3, :3].T
    side = float((g["bbox"][1] - g["bbox"][0]).max())
    tmax = float(np.abs(A).max())
    held("pose_rigid_xd", posed["v_pos"].cpu().numpy(), want_v, 1e-5 * tmax * side)
    e = np.concatenate([v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 1]], v[f[:, 0]] - v[f[:, 2]]])
    elen = np.linalg.norm(e.astype(np.float64), axis=1)
    emin = float(elen[elen > 0].min())
    ceil = ceilings(g)["normal"] + 16 * 2.0 ** -24 * float(np.abs(want_v).max()) / emin
    held("pose_rigid_normal", posed["v_nrm"].cpu().numpy(), want_n, ceil)


def test_implicit_pose_terms_keep_their_graph(g, dfm):
    """the weights come from the kernel, the dependence on tfs stays linear: d(sum R) / d tfs_j = the weights' column sums"""
    xc = T(g["xc"][:500])
    tfs0 = dfm.tfs
    try:
        dfm.tfs = tfs0.detach().clone().requires_grad_(True)
        J_inv = torch.eye(3, device=DEV).expand(500, 3, 3)
        valid = torch.ones(500, dtype=torch.bool, device=DEV)
        pts, R = dfm.implicit_pose_terms(xc, J_inv, valid)
        assert torch.equal(pts.detach(), xc)                 # the correction is zero in value
        R.sum().backward()
        grad = dfm.tfs.grad[0]
        w = dfm.query_weights(xc)
        want = torch.zeros_like(grad)
        want[:, :3, :3] = w.sum(0)[:, None, None]
        assert torch.allclose(grad, want, rtol=1e-5, atol=1e-6)
    finally:
        dfm.tfs = tfs0


def test_cli_poses_the_mesh_and_writes_the_animatable_form(tmp_path, golden_dir):
    """python -m intrinsicavatar_amd.mesh --smpl-npz BODY --pose-npz POSES --frame K --normals --skinned-npz OUT (in process): the
    .npz holds the canonical mesh + weights + the frame's transforms, and linear blend skinning of it in fp64 numpy gives the .obj"""
    import os
    from intrinsicavatar_amd import fields, io_formats, mesh
    z = np.load(os.path.join(golden_dir, "golden_smpl.npz"))
    body, poses = str(tmp_path / "body.npz"), str(tmp_path / "poses.npz")
    np.savez(body, **{k: z[k] for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "parents", "lbs_weights")}, betas=z["betas"][:1])
    np.savez(poses, body_pose=z["pose"][:, 3:], global_orient=z["pose"][:, :3], transl=z["transl"])
    geo = fields.VolumeSDF(seed=0)
    ck = str(tmp_path / "last.ckpt")
    torch.save({"state_dict": {f"model.geometry.{k}": v.detach().cpu() for k, v in geo.state_dict().items()}}, ck)
    obj, npz = str(tmp_path / "posed.obj"), str(tmp_path / "skinned.npz")
    assert mesh.main(["--state-dict", ck, "--smpl-npz", body, "--pose-npz", poses, "--frame", "2", "--resolution", "48", "--normals",
                      "--skinned-npz", npz, "--out", obj, "--device", DEV]) == 0
    v, f, n = io_formats.load_obj(obj, with_normals=True)
    a = np.load(npz)
    V = a["v_pos"].shape[0]
    assert V > 500 and v.shape == (V, 3) and n.shape == (V, 3) and np.array_equal(f, a["t_pos_idx"])
    assert a["weights"].shape == (V, 24) and np.abs(a["weights"].sum(1) - 1).max() < 1e-5 and a["tfs"].shape == (24, 4, 4)
    Tm = np.einsum("vj,jab->vab", a["weights"].astype(np.float64), a["tfs"].astype(np.float64))
    want = np.einsum("vab,vb->va", Tm[:, :3, :3], a["v_pos"].astype(np.float64)) + Tm[:, :3, 3]
    side = float(np.ptp(a["v_pos"], axis=0).max())
    assert np.abs(v - want).max() <= 1e-5 * max(1.0, float(np.abs(a["tfs"]).max())) * max(1.0, side)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-5
    assert (np.abs(n - normals_fp64(v, f)).max(1) <= normal_error_bound(v.astype(np.float64), f)).all()
    assert (np.abs(a["v_nrm"] - normals_fp64(a["v_pos"], f)).max(1) <= normal_error_bound(a["v_pos"].astype(np.float64), f)).all()
    # without --pose-npz the same command writes the canonical mesh, with or without normals
    plain = str(tmp_path / "cano.obj")
    assert mesh.main(["--state-dict", ck, "--smpl-npz", body, "--resolution", "48", "--normals", "--out", plain, "--device", DEV]) == 0
    v0, f0, n0 = io_formats.load_obj(plain, with_normals=True)
    assert np.array_equal(bits(v0), bits(a["v_pos"])) and np.array_equal(f0, f) and np.array_equal(bits(n0), bits(a["v_nrm"]))
