"""Plain torch reference of the hash-grid table backward (and of the forward it is the transpose of), its table layouts and its
input generators.  CPU only; nothing here imports the library.

As in tests/backward_refs.py a reference is ONE formula that runs in the dtype it is given: with float64 it is `ref64`, with
float32 the `twin32` whose distance from ref64 sets the tolerance of backward_refs.compare.  The twin adds its records one after
the other (index_add_ on the CPU), so it is a straightforward fp32 evaluation in every respect.

    grad[idx_c(l)] += gE[:, l] * w_c  +  gG[:, l] * sum_a q[a] * d w_c / d x_a         per level l and cell corner c

The corner index restates grid_index() of csrc/hashgrid.hip with explicit uint32 wrap-around (int64 values masked with
0xFFFFFFFF), so the negative cells of a point outside the unit cube and cells past the level's resolution index as the kernels do.
The level scale must be the fp32 value the kernels use: layouts come from oracle.hashgrid_offsets in the CPU tests and from
`layout()` below (make_cfg restated on the host's libm) in the GPU tests; the CPU test holds the two together.
"""
import ctypes
import ctypes.util
import functools
import struct

import torch

from tests import backward_refs as BR

M32 = 0xFFFFFFFF
BASE_RESOLUTION = 16
PER_LEVEL_SCALE = 1.447269237440378
SLICE = 8192                       # entries per slice of the binned backward (csrc/hashgrid.hip)

# name -> (n_levels, log2_hashmap_size): A the product's; odd5 all levels dense with sizes that are no power of two (partial last
# slice, modulo branch of grid_index, odd-count tail of the 16-byte pair load); one: the pair load never taken; small12: hashed
# from level 1 on, a table smaller than one slice, heavy collisions
CONFIGS = {"A": (16, 19), "odd5": (5, 19), "one": (1, 19), "small12": (6, 12)}
# the configuration ia_hashgrid_bwd_binned must REJECT (levels 5..7 have 128 slices): never run through the binned kernels
OVER_64_SLICES = dict(n_levels=8, F=2, n_features_per_level=2, log2_hashmap_size=20, base_resolution=16, per_level_scale=1.4473)


def cfg(name):
    """the configuration as a dict with the keys of both oracle.HASH_CFG ("F") and fields.HASH ("n_features_per_level")"""
    L, log2 = CONFIGS[name]
    return dict(n_levels=L, F=2, n_features_per_level=2, log2_hashmap_size=log2, base_resolution=BASE_RESOLUTION,
                per_level_scale=PER_LEVEL_SCALE)


def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


@functools.lru_cache(maxsize=None)
def _libm():
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for name, nargs in (("log2f", 1), ("exp2f", 1), ("ceilf", 1)):
        f = getattr(m, name)
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float] * nargs
    return m


def layout(c):
    """(total entries, offsets [L + 1], resolutions [L], fp32 scales [L] as Python floats) -- make_cfg of csrc/hashgrid.hip, on the
    host's libm in fp32 like the library's host code"""
    m = _libm()
    l2 = m.log2f(_f32(c["per_level_scale"]))
    offs, ress, scs, offset = [], [], [], 0
    for l in range(c["n_levels"]):
        sc = _f32(_f32(m.exp2f(_f32(float(l) * l2)) * float(c["base_resolution"])) - 1.0)
        res = int(m.ceilf(sc)) + 1
        p = min(res ** 3, M32 // 2)
        p = min((p + 7) // 8 * 8, 1 << c["log2_hashmap_size"])
        offs.append(offset); ress.append(res); scs.append(sc)
        offset += p
    offs.append(offset)
    return offset, offs, ress, scs


def n_slices(lay):
    """slices of 8192 entries per level"""
    _, offs, _, _ = lay
    return [(offs[l + 1] - offs[l] + SLICE - 1) // SLICE for l in range(len(offs) - 1)]


def _mul32(a, k):
    """(a * k) mod 2^32 for int64 a in [0, 2^32) without leaving int64"""
    return (a * (k & 0xFFFF) + (((a * (k >> 16)) & 0xFFFF) << 16)) & M32


def corner_index(hsize, res, px, py, pz):
    """grid_index() of csrc/hashgrid.hip; px, py, pz int64 in [0, 2^32) (uint32 values)"""
    stride, hashed = res & M32, False
    index = px
    if stride <= hsize:
        index = (index + py * stride) & M32
        stride = (stride * res) & M32
    else:
        hashed = True
    if not hashed and stride <= hsize:
        index = (index + pz * stride) & M32
        stride = (stride * res) & M32
    if hsize < stride:
        index = px ^ _mul32(py, 2654435761) ^ _mul32(pz, 805459861)
    return index % hsize


def _cells(x, sc, dtype):
    s = torch.tensor(sc, dtype=dtype)
    p = s * x + 0.5
    fl = torch.floor(p)
    return s, (fl.to(torch.int64) & M32), p - fl


def _corner(c, s, cell, f):
    """corner c of every point: (weight [n], its derivative along x, y, z [n, 3] WITHOUT q, uint32 cell coordinates)"""
    b = (c & 1, (c >> 1) & 1, (c >> 2) & 1)
    w = [f[:, d] if b[d] else 1.0 - f[:, d] for d in range(3)]
    sg = [s if b[d] else -s for d in range(3)]
    dw = torch.stack([sg[0] * w[1] * w[2], sg[1] * w[0] * w[2], sg[2] * w[0] * w[1]], -1)
    return w[0] * w[1] * w[2], dw, [(cell[:, d] + b[d]) & M32 for d in range(3)]


def table_grad(x, gE, gG, q, lay, dtype, levels=None):
    """the table gradient [entries * 2] of L = <gE, enc> + <gG, J q> in `dtype`; gE or (gG, q) may be None; levels: only these"""
    total, offs, ress, scs = lay
    x = x.to(dtype)
    out = torch.zeros(total, 2, dtype=dtype)
    for l in (range(len(ress)) if levels is None else levels):
        s, cell, f = _cells(x, scs[l], dtype)
        hsize = offs[l + 1] - offs[l]
        tab = out[offs[l]:offs[l + 1]]
        for c in range(8):
            w, dw, pc = _corner(c, s, cell, f)
            val = torch.zeros(x.shape[0], 2, dtype=dtype)
            if gE is not None:
                val = gE[:, 2 * l:2 * l + 2].to(dtype) * w[:, None]
            if gG is not None:
                val = val + gG[:, 2 * l:2 * l + 2].to(dtype) * (dw * q.to(dtype)).sum(-1, keepdim=True)
            tab.index_add_(0, corner_index(hsize, ress[l], *pc), val)
    return out.reshape(-1)


def forward(x, params, lay, dtype):
    """enc [n, 2 L] and J = d enc / d x [n, 2 L, 3] in `dtype`, with the index function of table_grad (differentiable in params)"""
    total, offs, ress, scs = lay
    x = x.to(dtype)
    tab_all = params.to(dtype).reshape(total, 2)
    enc, jac = [], []
    for l in range(len(ress)):
        s, cell, f = _cells(x, scs[l], dtype)
        hsize = offs[l + 1] - offs[l]
        e = torch.zeros(x.shape[0], 2, dtype=dtype)
        j = torch.zeros(x.shape[0], 2, 3, dtype=dtype)
        for c in range(8):
            w, dw, pc = _corner(c, s, cell, f)
            v = tab_all[offs[l] + corner_index(hsize, ress[l], *pc)]
            e = e + w[:, None] * v
            j = j + v[:, :, None] * dw[:, None, :]
        enc.append(e); jac.append(j)
    return torch.cat(enc, 1), torch.cat(jac, 1)


def level_slices(lay):
    """[(level, slice of the flat [entries * 2] table)]"""
    _, offs, _, _ = lay
    return [(l, slice(2 * offs[l], 2 * offs[l + 1])) for l in range(len(offs) - 1)]


# ----------------------------------------------------------------------------------------------------------------------
# inputs
N_FULL = 4099
GUARD_ULPS = 4.0


def near_lattice(x, scs):
    """rows with a coordinate that, on any level, lies within GUARD_ULPS fp32 ulps of a lattice plane: |p - round(p)| < 4 ulp32(p),
    p = sc x + 0.5 in fp64 from the fp32 scale (ulp32 taken at max(|p|, 0.5): the product sc x is rounded at that magnitude too).
    d w / d x jumps across such a plane, and a point that fp32 and fp64 place in different cells makes e32 meaningless."""
    xd = x.double()
    bad = torch.zeros(x.shape[0], dtype=torch.bool)
    for sc in scs:
        p = sc * xd + 0.5
        _, e = torch.frexp(p.abs().clamp(min=0.5))                 # |p| = m 2^e, m in [0.5, 1): ulp32 = 2^(e - 24)
        ulp = torch.ldexp(torch.ones_like(p), e - 24)
        bad |= ((p - torch.round(p)).abs() < GUARD_ULPS * ulp).any(-1)
    return bad


def _rays(g, n):
    """marching order: rays with step 0.004, 37 samples each, clipped to the cube (the existing binned test's points)"""
    per = 37
    n_r = (n + per - 1) // per
    o = torch.rand(n_r, 1, 3, generator=g) * 0.6 + 0.2
    d = torch.nn.functional.normalize(torch.randn(n_r, 1, 3, generator=g), dim=-1)
    return (o + d * (torch.arange(per)[None, :, None] * 0.004)).clamp(0.0, 1.0).reshape(-1, 3)[:n].contiguous()


def _special(g, n):
    from tests.forward_refs import HASH_SPECIAL
    assert n == len(HASH_SPECIAL)
    return torch.tensor(HASH_SPECIAL, dtype=torch.float32)


SAMPLERS = {
    "uniform": lambda g, n: torch.rand(n, 3, generator=g),
    "march": _rays,
    "same": lambda g, n: torch.rand(1, 3, generator=g).expand(n, 3).contiguous(),
    "alt2": lambda g, n: torch.rand(2, 3, generator=g)[torch.arange(n) % 2].contiguous(),
    "special": _special,                                                            # faces, corners, centre
    "near": lambda g, n: torch.rand(n, 3, generator=g) * 1.8 - 0.4,                 # outside the cube on some axes
    "far": lambda g, n: torch.rand(n, 3, generator=g) * 40.0 - 20.0,                # far outside: p ~ 8e4 on the fine levels
}
N_TWO_PARTS = 70_001                   # x 8 records on level 0 of A: two parts of at most 2^19 records
N_CLAMPED_PARTS = 64 * 65_536 + 129    # x 8 records in the one bucket of `one`: more than MAX_PARTS * PART_RECORDS
N_GUARD_CASE = 32_768 + 5              # past fields.HASH_BWD_BINNED_MIN
# (kind, n, seed, levels guarded) of every point set of the GPU file; the 4 M-point set serves configuration `one` alone, the last
# one the rejected configuration (scales of its own: guard_scales("over64"))
POINT_SETS = (("uniform", N_FULL, 11, 16), ("march", N_FULL, 12, 16), ("same", N_FULL, 13, 16), ("alt2", N_FULL, 14, 16),
              ("special", 8, 15, 16), ("near", 1000, 16, 16), ("far", 100, 17, 16), ("uniform", N_TWO_PARTS, 18, 16),
              ("uniform", N_CLAMPED_PARTS, 19, 1), ("uniform", N_GUARD_CASE, 20, "over64"))
MAX_ROUNDS = 64


def guard_scales(guard=16):
    """the scales a point set is guarded on: the first `guard` scales of configuration A (every configuration's levels are a prefix
    of A's: same base and per-level scale), or the scales of OVER_64_SLICES for "over64"."""
    if guard == "over64":
        return tuple(layout(OVER_64_SLICES)[3])
    return tuple(layout(cfg("A"))[3][:guard])


def make_points(kind, n, seed, guarded, guard_levels=16):
    """fp32 points [n, 3].  guarded (every case with the second-order term): a row near a lattice plane (near_lattice, on any of
    the first guard_levels levels) is RE-DRAWN from the same sampler, not left out, until none remains; rows of the `special` set are re-drawn
    uniformly.  Returns (x, rows re-drawn in the first round)."""
    g = BR.seeded(seed)
    x = SAMPLERS[kind](g, n).float()
    if not guarded:
        return x, 0
    first = None
    for rnd in range(MAX_ROUNDS + 1):
        bad = near_lattice(x, guard_scales(guard_levels))
        nb = int(bad.sum())
        first = nb if first is None else first
        if nb == 0:
            return x, first
        assert rnd < MAX_ROUNDS, f"{kind} n={n} seed={seed}: {nb} rows near a lattice plane after {MAX_ROUNDS} rounds"
        gr = BR.seeded(seed * 1000 + 17 + rnd)
        x[bad] = SAMPLERS["uniform" if kind == "special" else kind](gr, n).float()[bad]


def make_problem(kind, n, seed, guard_levels=16, n_levels=16):
    """x1: the points as drawn (first-order cases keep lattice points: the weights are continuous there); x2: guarded (cases with
    the second-order term); gE, gG [n, 2 L] and q [n, 3] ~ N(0, 1).  A configuration of fewer levels uses the first columns."""
    g = BR.seeded(seed + 500)
    x1, _ = make_points(kind, n, seed, False)
    x2, redrawn = make_points(kind, n, seed, True, guard_levels)
    return dict(kind=kind, n=n, x1=x1, x2=x2, redrawn=redrawn, gE=torch.randn(n, 2 * n_levels, generator=g),
                gG=torch.randn(n, 2 * n_levels, generator=g), q=torch.randn(n, 3, generator=g))


MODES = ("first", "both", "second")        # gE alone | gE and (gG, q) | (gG, q) alone, gE = NULL


def mode_inputs(p, mode, n=None, n_levels=16):
    """(x, gE or None, gG or None, q or None) of the first n rows for a configuration of n_levels levels"""
    n = p["n"] if n is None else n
    x = (p["x1"] if mode == "first" else p["x2"])[:n]
    gE = p["gE"][:n, :2 * n_levels] if mode != "second" else None
    gG = p["gG"][:n, :2 * n_levels] if mode != "first" else None
    return x, gE, gG, (p["q"][:n] if mode != "first" else None)


def refs(p, mode, lay, n=None, levels=None):
    """(ref64, twin32) of the table gradient"""
    x, gE, gG, q = mode_inputs(p, mode, n, len(lay[2]))
    return table_grad(x, gE, gG, q, lay, torch.float64, levels), table_grad(x, gE, gG, q, lay, torch.float32, levels)
