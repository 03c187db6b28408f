"""GPU (MI355X): the scalar-served voxel cells of the early-filter search (broyden_spec_kernel, grid_sample_J's SCELLS, csrc/snarf.hip).
IA_BR_SPEC_SCALAR = 1 (the default) serves the lanes in the voxel cell of the wave's first active lane from one wave-uniform scalar load,
= 0 loads every lane's corners through the vector path.  The same bytes go into the same packed multiply-adds with each lane's own
weights, so both must agree bit for bit -- with each other and with the exact
small-batch path (broyden_items_rows_kernel, plain loads) -- on point sets built to stress the group logic: every lane of a wave in one
cell, no two lanes in one cell, cells on each grid face with one x-corner outside, points far outside the grid, non-finite points
mixed into the waves, and the march points of the headline frame."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def frame():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from tools import spec_search_probe as SP
    from intrinsicavatar_amd import synthetic as S
    rs, rays, _ = S.build_frame(DEV, 128, 128, pose_seed=0, beta=0.01)
    pts = SP.march_points(rs, rays, 1 << 15)
    return SP, rs, pts


def _posed(dfm, g):
    """posed points whose FIRST search (the highest init) starts at grid coordinates g [P, 3] (g in [-1, 1] spans the grid)."""
    xc = g / dfm.scale_kernel - dfm.offset_kernel
    T = dfm.tfs[0, int(dfm.init_bones[-1])]
    return (xc @ T[:3, :3].T + T[:3, 3]).contiguous()


def _point_sets(dfm, march):
    _, _, D, H, W = dfm.lbs_voxel_final.shape
    dims = torch.tensor([W, H, D], device=DEV, dtype=torch.float32)
    gen = torch.Generator(device=DEV).manual_seed(7)
    sets = {}
    # every lane of a wave in one cell: one march point repeated, and jittered well inside its cell
    p = march[12345]
    sets["one_cell"] = p.expand(4096, 3).contiguous()
    sets["one_cell_jitter"] = (p + 1e-6 * torch.randn((4096, 3), device=DEV, generator=gen)).contiguous()
    # no two lanes in one cell: a lattice 1.5 cells apart, visited in a scrambled order
    step = 1.5 * 2.0 / (dims - 1)
    ax = [torch.arange(-0.95, 0.95, float(step[a]), device=DEV) for a in range(3)]
    lat = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    lat = lat[torch.randperm(lat.shape[0], device=DEV, generator=gen)[:16384]]
    sets["distinct_cells"] = _posed(dfm, lat)
    # cells on each grid face: the face itself, half a cell inside (x0 = dim-2 / x0 = 0), half a cell outside (x1 or x0 out of range)
    face = []
    for a in range(3):
        h = 1.0 / (dims[a] - 1)
        for v in (-1.0 - h, -1.0, -1.0 + h, 1.0 - h, 1.0, 1.0 + h):
            g = torch.rand((1024, 3), device=DEV, generator=gen) * 2 - 1
            g[:, a] = v
            face.append(g)
    sets["faces"] = _posed(dfm, torch.cat(face)[torch.randperm(18 * 1024, device=DEV, generator=gen)])
    # far outside the grid (a few grid sizes up to 1e30), mixed with march points
    far = torch.randn((4096, 3), device=DEV, generator=gen) * torch.logspace(0.5, 30, 4096, device=DEV)[:, None]
    mix = torch.stack([far, march[:4096]], 1).reshape(-1, 3)
    sets["far"] = mix.contiguous()
    # non-finite coordinates, one per lane pair, so that waves hold both kinds (and the wave's first lane is the non-finite one)
    bad = march[4096:8192].clone()
    bad[0::3, 0] = float("nan")
    bad[1::3, 1] = float("inf")
    bad[2::3, 2] = float("-inf")
    sets["non_finite"] = torch.stack([bad, march[8192:12288]], 1).reshape(-1, 3).contiguous()
    sets["march"] = march[:200_000].contiguous()
    return sets


def _run(dfm, pts, monkeypatch, scalar, small):
    monkeypatch.setenv("IA_BR_SPEC_SCALAR", str(scalar))
    if small:
        monkeypatch.delenv("IA_BR_SMALL_MAX", raising=False)          # default: batches up to 2^18 points take the exact path
    else:
        monkeypatch.setenv("IA_BR_SMALL_MAX", "0")                    # every batch through broyden_spec_kernel
    r = dfm._candidates(pts, with_src=True, want_fwd=True, want_jinv=True)
    torch.cuda.synchronize()
    return r


def _same(a, b, tag):
    assert a[4] == b[4], (tag, a[4], b[4])
    for k in (0, 1, 2, 3):                                              # cand_x, cand_src, cnt, start
        assert torch.equal(a[k].view(torch.int32) if a[k].is_floating_point() else a[k],
                           b[k].view(torch.int32) if b[k].is_floating_point() else b[k]), (tag, k)
    src = a[1].long()
    for k in (5, 6):                                                    # fwd_J, J_inv of every candidate
        x, y = a[k].reshape(-1, 9)[src], b[k].reshape(-1, 9)[src]
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (tag, k)


@pytest.mark.parametrize("name", ["one_cell", "one_cell_jitter", "distinct_cells", "faces", "far", "non_finite", "march"])
def test_scalar_cells_are_the_vector_path_bit_for_bit(frame, monkeypatch, name):
    SP, rs, march = frame
    dfm = rs.deformer
    pts = _point_sets(dfm, march)[name]
    want = _run(dfm, pts, monkeypatch, 0, small=False)
    _same(_run(dfm, pts, monkeypatch, 1, small=False), want, name)


@pytest.mark.parametrize("name", ["one_cell", "one_cell_jitter", "distinct_cells", "faces", "far", "non_finite", "march"])
def test_scalar_cells_are_the_exact_small_batch_path(frame, monkeypatch, name):
    SP, rs, march = frame
    dfm = rs.deformer
    pts = _point_sets(dfm, march)[name]
    exact = _run(dfm, pts, monkeypatch, 1, small=True)
    for scalar in (0, 1):
        _same(_run(dfm, pts, monkeypatch, scalar, small=False), exact, (name, scalar))


def test_scalar_cells_counters_and_full_outputs(frame, monkeypatch):
    """the entry point with per-init outputs (ia_fuse_broyden_spec: x, is_valid) and the counting instantiation."""
    SP, rs, march = frame
    dfm = rs.deformer
    pts = torch.cat([_point_sets(dfm, march)[k] for k in ("faces", "non_finite", "march")])
    out = {}
    for scalar in (0, 1):
        monkeypatch.setenv("IA_BR_SPEC_SCALAR", str(scalar))
        cnt = torch.zeros(5, dtype=torch.int64, device=DEV)
        x, v = SP.search(dfm, pts, 1e-3, counters=cnt)
        x2, v2 = SP.search(dfm, pts, 1e-3)
        out[scalar] = (torch.where(v[..., None], x, torch.zeros_like(x)), v, cnt, torch.where(v2[..., None], x2, torch.zeros_like(x2)), v2)
    for k in range(5):
        a, b = out[1][k], out[0][k]
        assert torch.equal(a.view(torch.int32) if a.is_floating_point() else a, b.view(torch.int32) if b.is_floating_point() else b), k


def test_scalar_cells_on_the_sdf_only_path_through_a_permutation(frame, monkeypatch):
    """the secondary march's call: SDF-only candidates in the split layout, points evaluated through a permutation, and the
    min-over-candidates SDF (deform_sdf) -- bit for bit with the leader cell on and off."""
    SP, rs, march = frame
    dfm = rs.deformer
    pts = march[:200_000].contiguous()
    order = torch.randperm(pts.shape[0], device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)).to(torch.int32)
    monkeypatch.setenv("IA_BR_SMALL_MAX", "0")
    out = {}
    for scalar in (0, 1):
        monkeypatch.setenv("IA_BR_SPEC_SCALAR", str(scalar))
        c = dfm._candidates(pts, with_src=False, order=order, split=True)
        s = dfm.deform_sdf(pts, rs.geometry, order=order)
        torch.cuda.synchronize()
        split = [t for t in (c[7] or ()) + (c[8],) if torch.is_tensor(t)]          # first_pos, tile offsets, n_first
        out[scalar] = (c[4], [c[0], c[2], c[3], s] + split)
    assert out[1][0] == out[0][0]
    for a, b in zip(out[1][1], out[0][1]):
        assert torch.equal(a.view(torch.int32) if a.is_floating_point() else a, b.view(torch.int32) if b.is_floating_point() else b)
