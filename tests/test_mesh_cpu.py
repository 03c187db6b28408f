"""Mesh export without a GPU: the marching-cubes arithmetic of intrinsicavatar_amd/csrc/mc_math.h replayed on the host by
tests/mc_harness.c (table-independent mesh properties on analytic grids, the tie rule, empty / full / 2^3 / non-cubic grids), the OBJ
writer, and the host-side float32 chains of BaseImplicitGeometry.isosurface (grid axes, two-pass bbox)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mc") / "libmc_harness.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-fvisibility=hidden", "-o", so,
                           os.path.join(HERE, "mc_harness.c"), "-lm"])
    return C.CDLL(so)


def mc_host(h, level, threshold=0.0, vmin=(0.0, 0.0, 0.0), vmax=(1.0, 1.0, 1.0)):
    """the product's extraction on the host: (v_pos float32 [V,3], t_pos_idx int64 [T,3])."""
    lv = np.ascontiguousarray(level, dtype=np.float32)
    nx, ny, nz = lv.shape
    cnt = np.zeros(2, np.int64)
    vp = C.c_void_p
    h.mc_h_count(C.c_int(nx), C.c_int(ny), C.c_int(nz), vp(lv.ctypes.data), C.c_float(threshold), vp(cnt.ctypes.data))
    v = np.zeros((int(cnt[0]), 3), np.float32)
    f = np.zeros((int(cnt[1]), 3), np.int64)
    box = np.array(list(vmin) + list(vmax), np.float32)
    assert h.mc_h_fill(C.c_int(nx), C.c_int(ny), C.c_int(nz), vp(lv.ctypes.data), C.c_float(threshold), vp(box.ctypes.data),
                       vp(v.ctypes.data), vp(f.ctypes.data)) == 0
    return v, f


def grid(shape, lo=-1.0, hi=1.0):
    axes = [np.linspace(lo, hi, n) for n in shape]
    return np.meshgrid(*axes, indexing="ij")


def analytic(name, R=64):
    X, Y, Z = grid((R, R, R))
    if name == "sphere":
        return np.sqrt(X ** 2 + Y ** 2 + Z ** 2) - 0.6, 4 / 3 * np.pi * 0.6 ** 3, 2
    if name == "torus":
        return np.sqrt((np.sqrt(X ** 2 + Y ** 2) - 0.5) ** 2 + Z ** 2) - 0.2, 2 * np.pi ** 2 * 0.5 * 0.2 ** 2, 0
    if name == "two_spheres":
        a = np.sqrt((X + 0.45) ** 2 + Y ** 2 + Z ** 2) - 0.35
        b = np.sqrt((X - 0.45) ** 2 + (Y - 0.1) ** 2 + Z ** 2) - 0.3
        return np.minimum(a, b), 4 / 3 * np.pi * (0.35 ** 3 + 0.3 ** 3), 4
    if name == "box":
        q = np.abs(np.stack([X, Y, Z])) - np.array([0.5, 0.3, 0.7])[:, None, None, None]
        out = np.linalg.norm(np.maximum(q, 0), axis=0) + np.minimum(q.max(0), 0)
        return out, 8 * 0.5 * 0.3 * 0.7, 2
    raise KeyError(name)


def edge_counts(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, cnt = np.unique(e, axis=0, return_counts=True)
    return cnt


def euler(v, f):
    return len(v) - len(edge_counts(f)) + len(f)


def directed_pairs_ok(f):
    """every directed edge appears once and its reverse once: a consistently oriented closed 2-manifold (edge-wise)"""
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = d[:, 0] * (d.max() + 1) + d[:, 1]
    rkey = d[:, 1] * (d.max() + 1) + d[:, 0]
    return len(np.unique(key)) == len(key) and np.array_equal(np.sort(key), np.sort(rkey))


def signed_volume(v, f):
    p = v.astype(np.float64)
    return float(np.einsum("ij,ij->i", p[f[:, 0]], np.cross(p[f[:, 1]], p[f[:, 2]])).sum() / 6)


def crossed_edges(level, threshold):
    """[(i, j, k, axis)] of every crossed grid edge in the stated vertex order (owning point C order, then axis)"""
    ins = -level.astype(np.float32) > np.float32(threshold)
    out = []
    for a in range(3):
        sl0 = [slice(None)] * 3
        sl1 = [slice(None)] * 3
        sl0[a] = slice(0, -1)
        sl1[a] = slice(1, None)
        c = ins[tuple(sl0)] != ins[tuple(sl1)]
        for idx in np.argwhere(c):
            out.append((*idx, a))
    nx, ny, nz = level.shape
    out.sort(key=lambda e: (((e[0] * ny) + e[1]) * nz + e[2], e[3]))
    return out


def expected_vertices(level, threshold, vmin, vmax):
    """the stated vertex convention, restated in numpy: index + t (t in float64) rounded to float32, / (n - 1), * (vmax - vmin) + vmin"""
    lv = level.astype(np.float32)
    n = lv.shape
    rows = []
    for (i, j, k, a) in crossed_edges(lv, threshold):
        idx = [i, j, k]
        q = list(idx)
        q[a] += 1
        f0, f1 = -np.float64(lv[i, j, k]), -np.float64(lv[tuple(q)])
        t = (np.float64(np.float32(threshold)) - f0) / (f1 - f0)
        c = [np.float32(x) for x in idx]
        c[a] = np.float32(np.float64(idx[a]) + t)
        row = []
        for ax in range(3):
            v = np.float32(c[ax] / np.float32(n[ax] - 1))
            d = np.float32(np.float32(vmax[ax]) - np.float32(vmin[ax]))
            row.append(np.float32(np.float32(v * d) + np.float32(vmin[ax])))
        rows.append(row)
    return np.array(rows, np.float32).reshape(-1, 3)


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres", "box"])
def test_analytic_surfaces(harness, name):
    level, volume, chi = analytic(name)
    v, f = mc_host(harness, level, 0.0, (-1, -1, -1), (1, 1, 1))
    assert len(f) > 0
    assert (edge_counts(f) == 2).all(), "an edge is not shared by exactly two faces"
    assert directed_pairs_ok(f)
    assert euler(v, f) == chi
    assert len(np.unique(f)) == len(v), "every vertex belongs to a face"
    # every vertex on its crossed edge, one vertex per crossed edge, in the stated order, bit for bit
    assert np.array_equal(v, expected_vertices(level, 0.0, (-1, -1, -1), (1, 1, 1)))
    vol = signed_volume(v, f)
    assert vol > 0, "faces must point toward increasing level"
    assert abs(vol - volume) < 0.02 * volume, (vol, volume)


def test_vertices_lie_on_crossed_edges(harness):
    level, _, _ = analytic("torus", 24)
    R = level.shape[0]
    v, f = mc_host(harness, level, 0.0, (0, 0, 0), (R - 1, R - 1, R - 1))        # index coordinates (up to one rounding)
    edges = crossed_edges(level.astype(np.float32), 0.0)
    assert len(edges) == len(v)
    for (i, j, k, a), p in zip(edges, v.astype(np.float64)):
        base = np.array([i, j, k], np.float64)
        off = np.abs(p - base)
        others = [c for c in range(3) if c != a]
        assert (off[others] < 1e-5).all()
        assert -1e-5 <= p[a] - base[a] <= 1 + 1e-5


def test_noise_field_is_closed_and_oriented(harness):
    rng = np.random.default_rng(3)
    lv = rng.standard_normal((23, 19, 17)).astype(np.float32)
    lv[[0, -1]] = 1
    lv[:, [0, -1]] = 1
    lv[:, :, [0, -1]] = 1                      # positive (outside) boundary: every component closes inside the grid
    v, f = mc_host(harness, lv)
    assert (edge_counts(f) == 2).all() and directed_pairs_ok(f)
    assert signed_volume(v, f) > 0
    assert np.array_equal(v, expected_vertices(lv, 0.0, (0, 0, 0), (1, 1, 1)))
    ins = (-lv > 0).astype(np.int64)
    order = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
    ci = sum(ins[dx:dx + 22, dy:dy + 18, dz:dz + 16] << b for b, (dx, dy, dz) in enumerate(order))
    cubes = np.unique(ci)
    assert len(cubes) > 100


def test_tie_rule_threshold_equal_is_outside(harness):
    thr = 0.25
    lv = np.ones((5, 5, 5), np.float32)
    lv[2, 2, 2] = -thr                          # f == threshold: outside -> no surface
    v, f = mc_host(harness, lv, thr)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    lv[2, 2, 2] = np.nextafter(np.float32(-thr), np.float32(-1))     # f just above the threshold: inside
    v, f = mc_host(harness, lv, thr)
    assert len(v) == 6 and len(f) == 8 and euler(v, f) == 2
    assert (v == 0.5).all()                     # t rounds to the inside point itself: 2 / 4 on every axis
    # a neighbour exactly at the threshold is outside: the vertex lands exactly on it (t = 1)
    lv = np.ones((5, 5, 5), np.float32)
    lv[2, 2, 2] = -1.0
    lv[3, 2, 2] = -thr
    v, f = mc_host(harness, lv, thr, (0, 0, 0), (4, 4, 4))
    assert len(v) == 6
    assert [3.0, 2.0, 2.0] in v.tolist()


def test_empty_full_and_single_cell(harness):
    for fill in (1.0, -1.0):
        v, f = mc_host(harness, np.full((6, 7, 8), fill, np.float32))
        assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == np.float32 and f.dtype == np.int64
    # R = 2: every one of the 256 cube cases -> one vertex per crossed edge, the table's triangle count, all vertices used
    order = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
    n_tri = []
    for cube in range(256):
        lv = np.ones((2, 2, 2), np.float32)
        for b, c in enumerate(order):
            if cube >> b & 1:
                lv[c] = -1.0
        v, f = mc_host(harness, lv)
        assert len(v) == len(crossed_edges(lv, 0.0))
        if 0 < cube < 255:
            assert len(f) >= 1 and set(np.unique(f)) == set(range(len(v)))
        assert ((v >= 0) & (v <= 1)).all()
        n_tri.append(len(f))
    assert n_tri[0] == n_tri[255] == 0 and max(n_tri) <= 5


def test_non_cubic_grid(harness):
    X, Y, Z = grid((40, 24, 17))
    level = np.sqrt((X / 0.8) ** 2 + (Y / 0.6) ** 2 + (Z / 0.7) ** 2) - 1.0
    v, f = mc_host(harness, level, 0.0, (-1, -1, -1), (1, 1, 1))
    assert (edge_counts(f) == 2).all() and directed_pairs_ok(f) and euler(v, f) == 2
    assert np.array_equal(v, expected_vertices(level, 0.0, (-1, -1, -1), (1, 1, 1)))
    vol = signed_volume(v, f)
    assert abs(vol - 4 / 3 * np.pi * 0.8 * 0.6 * 0.7) < 0.05 * vol


def test_obj_round_trip(tmp_path):
    from intrinsicavatar_amd import io_formats
    rng = np.random.default_rng(0)
    v = (rng.standard_normal((500, 3)) * np.array([1e-7, 1.0, 3e4])).astype(np.float32)
    v[0] = [np.float32(1) / 3, -0.0, np.finfo(np.float32).tiny]
    f = rng.integers(0, 500, (777, 3)).astype(np.int64)
    path = tmp_path / "m.obj"
    io_formats.save_obj(str(path), torch.from_numpy(v), torch.from_numpy(f))
    lines = path.read_text().splitlines()
    assert lines[0].startswith("v ") and lines[500].startswith("f ")
    assert [int(t) for t in lines[500].split()[1:]] == (f[0] + 1).tolist()
    v2, f2 = io_formats.load_obj(str(path))
    assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(f2, f)
    io_formats.save_obj(str(tmp_path / "e.obj"), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    v3, f3 = io_formats.load_obj(str(tmp_path / "e.obj"))
    assert v3.shape == (0, 3) and f3.shape == (0, 3)


def _reference_fine_bbox(v_pos, bbox_cpu):
    """BaseImplicitGeometry.isosurface (rf/geometry.py:94-104), as written there"""
    vmin, vmax = v_pos.amin(dim=0), v_pos.amax(dim=0)
    vmin_ = (vmin - (vmax - vmin) * 0.1).clamp(bbox_cpu[0], bbox_cpu[1])
    vmax_ = (vmax + (vmax - vmin) * 0.1).clamp(bbox_cpu[0], bbox_cpu[1])
    return vmin_, vmax_


def test_two_pass_bbox_arithmetic():
    from intrinsicavatar_amd import mesh
    bbox = torch.tensor([[-1.1, -1.3, -0.4], [0.9, 1.2, 0.35]], dtype=torch.float32)
    rng = np.random.default_rng(5)
    sets = [torch.tensor([[-1.0, -1.2, -0.3], [0.8, 1.1, 0.3]]),                       # expansion clamped on every side
            torch.tensor([[-0.2, 0.1, 0.0], [0.3, 0.2, 0.1], [0.0, 0.15, 0.05]]),       # free expansion
            torch.tensor([[-1.1, 0.0, 0.0], [-1.1, 0.0, 0.0]]),                         # degenerate extent on the bbox boundary
            torch.from_numpy(rng.uniform(-1, 1, (1000, 3)).astype(np.float32) * np.float32(0.4))]
    for v in sets:
        v = v.float()
        got = mesh.fine_bbox(v.amin(0), v.amax(0), bbox)
        ref = _reference_fine_bbox(v, bbox)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
        # float32 restatement: extent, times 0.1f, expand, clamp
        lo, hi = v.amin(0).numpy(), v.amax(0).numpy()
        d = (hi - lo).astype(np.float32) * np.float32(0.1)
        b = bbox.numpy()
        assert np.array_equal(got[0].numpy(), np.clip((lo - d).astype(np.float32), b[0], b[1]))
        assert np.array_equal(got[1].numpy(), np.clip((hi + d).astype(np.float32), b[0], b[1]))


def _reference_points(R, vmin, vmax):
    """isosurface_'s point chain on the host: linspace(0, 1, R) meshgrid (ij), then scale_anything per axis"""
    x = torch.linspace(0, 1, R)
    g = torch.meshgrid(x, x, x, indexing="ij")
    verts = torch.cat([g[0].reshape(-1, 1), g[1].reshape(-1, 1), g[2].reshape(-1, 1)], dim=-1).reshape(-1, 3)
    sa = lambda d, lo, hi: ((d - 0) / (1 - 0)) * (hi - lo) + lo      # noqa: E731  models/utils.py scale_anything
    return torch.stack([sa(verts[..., a], vmin[a], vmax[a]) for a in range(3)], dim=-1)


def test_grid_axes_match_the_reference_point_chain():
    from intrinsicavatar_amd import mesh
    bbox = torch.tensor([[-1.1, -1.3, -0.4], [0.9, 1.2, 0.35]], dtype=torch.float32)
    for R in (2, 7, 33):
        # coarse pass: the reference hands numpy float32 scalars (bbox.numpy()); fine pass: float32 0-d tensors
        ref = _reference_points(R, bbox.numpy()[0], bbox.numpy()[1])
        vmin_, vmax_ = mesh.fine_bbox(torch.tensor([-0.5, -0.7, -0.1]), torch.tensor([0.4, 0.9, 0.2]), bbox)
        ref_fine = _reference_points(R, vmin_, vmax_)
        for (lo, hi), r in (((bbox[0], bbox[1]), ref), ((vmin_, vmax_), ref_fine)):
            ax = mesh.grid_axes(R, lo, hi)
            assert ax.dtype == torch.float32 and ax.shape == (3, R)
            i, j, k = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")
            pts = torch.stack([ax[0][i.reshape(-1)], ax[1][j.reshape(-1)], ax[2][k.reshape(-1)]], -1)
            assert torch.equal(pts, r)


def test_volume_sdf_keeps_its_bbox():
    from intrinsicavatar_amd import fields
    geo = fields.VolumeSDF(seed=0)
    bbox = torch.tensor([[-1.0, -1.2, -0.3], [0.9, 0.8, 0.35]])
    geo.prepare_bbox(bbox)
    assert torch.equal(geo.bbox, bbox)
    assert torch.equal(geo.center, (bbox[0] + bbox[1]) / 2) and torch.equal(geo.scale, bbox[1] - bbox[0])
    assert callable(geo.isosurface)
