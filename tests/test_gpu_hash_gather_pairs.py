"""GPU: the feature-only level-major hash gather (`ia_hashgrid_fwd_xcd` without Jacobian) against the flat kernel, bit for bit, on
point sets built by hand around the corner loads it shares between the two x-neighbours.

On a dense level the gather reads both x-neighbours of a cell edge with ONE 16-byte load at entry i0; on a hashed level it reads the
aligned entry pair that holds i0, which also holds i1 = i0 ^ 1 when the cell's x is even, and takes i1 from a load of its own
otherwise.  What can go wrong is therefore decided by the PARITY of the cell's x at each level, by where i0 sits in its 128-byte
line, by the wrap of the dense index at the upper faces, and by which lanes carry a second point.  The sets below pin those, level by
level: the per-level scale moves a point's cell, so every set is built for ONE target level and its parity is asserted there with
the kernel's own arithmetic (p = fma(scale, x, 0.5), cell = floor(p)); all 16 levels are compared every time.

The table holds distinct values (entry k = (k + 1) 2^-20), so a wrong entry cannot pass by coincidence."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 63, 64, 65, 129, 257)                    # below, at and above one wave; more than one wave; more than one workgroup
BLOCK = 8192                                         # points per (workgroup per CU) of one XCD slot: the lane stride is a multiple of it


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def grid(oracle):
    from intrinsicavatar_amd import build
    build.build()
    from intrinsicavatar_amd import fields
    total, offs, res, sc = oracle.hashgrid_offsets()
    assert total == fields.hash_n_entries() and 2 * total < 1 << 24          # distinct float32 values below
    params = T((np.arange(1, 2 * total + 1, dtype=np.float64) * 2.0 ** -20).astype(np.float32))
    hashed = np.array([int(res[l]) ** 3 > int(offs[l + 1] - offs[l]) for l in range(len(res))])
    assert list(np.where(hashed)[0]) == list(range(5, 16))                   # the shipped HASH config: 5 dense, 11 hashed levels
    return dict(fields=fields, params=params, offs=offs.astype(np.int64), res=res.astype(np.int64), sc=sc, hashed=hashed)


def cells(x, sc_l):
    """cell coordinates as the kernels compute them: floor(fma(scale, x, 0.5)) (the product of two float32 is exact in float64)"""
    p = (np.float64(sc_l) * x.astype(np.float64) + 0.5).astype(np.float32)
    return np.floor(p).astype(np.int64)


def in_cells(c, sc_l, rng):
    """points inside the cells c [n,3] of one level, away from the cell walls"""
    u = rng.uniform(0.55, 0.9, c.shape)
    x = ((c + u - 0.5) / np.float64(sc_l)).astype(np.float32)
    assert np.array_equal(cells(x, sc_l), c) and (x >= 0).all() and (x <= 1).all()
    return x


def random_cells(n, g, l, rng):
    top = int(np.floor(g["sc"][l])) - 1                                      # cell coordinates 0 .. top keep the point inside the cube
    return rng.integers(0, top + 1, (n, 3)), top


def with_parity(n, g, l, rng, parity):
    """n in-cube points whose cell x at level l has the given parity [n]"""
    c, top = random_cells(n, g, l, rng)
    c[:, 0] = np.minimum(c[:, 0] // 2 * 2 + parity, top - (top - parity) % 2)
    x = in_cells(c, g["sc"][l], rng)
    assert np.array_equal(cells(x, g["sc"][l])[:, 0] & 1, parity)
    return x


def line_end(n, g, l, rng):
    """cell x at the last entry of a 128-byte line (16 entries): on a dense level the absolute entry index of corner (x, y, z) is
    15 mod 16, so the 16-byte pair load straddles two lines; on a hashed level x = 15 mod 16, so x + 1 carries out of the line"""
    c, top = random_cells(n, g, l, rng)
    res, off = int(g["res"][l]), int(g["offs"][l])
    if g["hashed"][l]:
        c[:, 0] = np.minimum(c[:, 0] // 16 * 16 + 15, (top + 1) // 16 * 16 - 1)
        assert (c[:, 0] % 16 == 15).all() and (c[:, 0] >= 0).all()
        return in_cells(c, g["sc"][l], rng)
    want = (15 - (off + res * (c[:, 1] + res * c[:, 2]))) % 16               # 0 .. 15
    face = want > top                                                        # level 0 (16 cells a row, 15 of them inside): x = 1
    c[:, 0] = np.minimum(want, top)
    x = in_cells(c, g["sc"][l], rng)
    x[face, 0] = 1.0
    c = cells(x, g["sc"][l])
    assert ((off + c[:, 0] + res * (c[:, 1] + res * c[:, 2])) % 16 == 15).all()
    return x


def upper_faces(n, g, l, rng):
    """cells along x on the upper y / z faces: there the dense index passes the table size and wraps, and for one cell the table's
    last entry and its first are x-neighbours"""
    c, top = random_cells(n, g, l, rng)
    c[:, 0] = np.arange(n) % (top + 1)
    x = in_cells(c, g["sc"][l], rng)
    x[:, 1] = 1.0
    x[:, 2] = np.where(np.arange(n) // (top + 1) % 2 == 0, 1.0, x[:, 2])
    return x


def off_cube(n, rng, kind):
    if kind == "faces":
        vals = np.array([0.0, 1.0, 0.5, 0.999999, 1e-7, 0.25], np.float32)
        return vals[rng.integers(0, len(vals), (n, 3))]
    if kind == "outside":
        return (rng.random((n, 3)) * 1.8 - 0.4).astype(np.float32)
    return (rng.random((n, 3)) * 40.0 - 20.0).astype(np.float32)            # far outside


def both(g, x, monkeypatch):
    out = {}
    for m in ("flat", "xcd"):
        monkeypatch.setenv("IA_HASH_FWD", m)
        out[m] = g["fields"].hashgrid_forward(T(x), g["params"], with_jac=False)
    monkeypatch.delenv("IA_HASH_FWD")
    return out["flat"], out["xcd"]


def assert_same(g, x, monkeypatch, what):
    flat, xcd = both(g, x, monkeypatch)
    if not torch.equal(flat, xcd):
        bad = (flat != xcd).nonzero()
        p, col = int(bad[0, 0]), int(bad[0, 1])
        raise AssertionError(f"{what}: {bad.shape[0]} values differ; first at point {p} {x[p].tolist()} level {col // 2}: "
                             f"flat {float(flat[p, col])!r} level-major {float(xcd[p, col])!r}")


PARITY = {
    "every point in an even-x cell": lambda n: np.zeros(n, np.int64),
    "every point in an odd-x cell": lambda n: np.ones(n, np.int64),
    "parity alternating lane by lane": lambda n: np.arange(n) & 1,
    "parity alternating wave by wave": lambda n: np.arange(n) // 64 & 1,
}


@pytest.mark.parametrize("kind", list(PARITY))
def test_cell_parity_sets_equal_the_flat_kernel_bit_for_bit(grid, monkeypatch, kind):
    """at these sizes the lane stride exceeds the batch, so every lane carries ONE point (`two == false` in every wave)"""
    rng = np.random.default_rng(11)
    for n in SIZES:
        for l in range(16):
            assert_same(grid, with_parity(n, grid, l, rng, PARITY[kind](n)), monkeypatch, f"{kind}, n {n}, built for level {l}")


@pytest.mark.parametrize("kind", ["x at the last cell before a 16-entry line boundary", "cells along x on the upper faces"])
def test_line_ends_and_upper_faces_equal_the_flat_kernel_bit_for_bit(grid, monkeypatch, kind):
    rng = np.random.default_rng(12)
    make = line_end if kind.startswith("x at") else upper_faces
    for n in SIZES:
        for l in range(16):
            assert_same(grid, make(n, grid, l, rng), monkeypatch, f"{kind}, n {n}, built for level {l}")


@pytest.mark.parametrize("kind", ["faces", "outside", "far outside"])
def test_points_on_and_outside_the_cube_equal_the_flat_kernel_bit_for_bit(grid, monkeypatch, kind):
    """on the faces, outside and far outside the unit cube: the dense levels redo these with the full modulo"""
    rng = np.random.default_rng(13)
    for n in SIZES:
        assert_same(grid, off_cube(n, rng, kind), monkeypatch, f"{kind}, n {n}")


@pytest.mark.parametrize("n", [13 * BLOCK + 77, 400_003])
def test_two_points_per_lane_equal_the_flat_kernel_bit_for_bit(grid, monkeypatch, n):
    """batches above the lane stride (a multiple of 8192 points): a lane gathers points i and i + stride together.  13 x 8192 + 77 points
    take the small-batch schedule (every point through one XCD slot per hashed level), 400 003 the one-table-per-launch schedule of
    the headline step (an eighth of the points per slot).  Parity in blocks of 4 x 8192 points pairs even with odd cells in one
    lane for every stride of 4 to 7 blocks; parity drawn per point gives all four combinations; the last points of a share have no
    partner (`two == false`); points on the faces, at line ends and outside the cube ride along."""
    rng = np.random.default_rng(14)
    for l in (0, 2, 4, 5, 8, 12, 15):
        blocks = np.arange(n) // (4 * BLOCK) & 1
        x = with_parity(n, grid, l, rng, blocks)
        c = cells(x, grid["sc"][l])[:, 0] & 1
        for k in (4, 5, 6, 7):
            assert (c[: n - k * BLOCK] != c[k * BLOCK:]).any()
        assert_same(grid, x, monkeypatch, f"parity in blocks, n {n}, built for level {l}")
        x = with_parity(n, grid, l, rng, rng.integers(0, 2, n))
        x[1000:3000] = line_end(2000, grid, l, rng)
        x[3000:5000] = upper_faces(2000, grid, l, rng)
        x[5000:6000] = off_cube(1000, rng, "faces")
        x[6000:9000] = off_cube(3000, rng, "outside")
        x[9000:9100] = off_cube(100, rng, "far outside")
        assert_same(grid, x, monkeypatch, f"parity per point, n {n}, built for level {l}")
