"""GPU: the two hash-grid table backward paths, ia_hashgrid_bwd (run-merged atomics) and ia_hashgrid_bwd_binned (count, scan, staged
fill, fixed-point LDS reduce), through the C ABI with strides, mask and scratch of the test's own, against the fp64 torch
reference of tests/hash_bwd_refs.py (checked on the CPU by tests/test_hash_bwd_refs_cpu.py).

Comparison: backward_refs.compare unchanged, max|got - ref64| <= max(16 * e32, 32 ulp of max|ref64|), applied once PER LEVEL on
that level's slice of the table -- a fine level, whose e32 is set by ulp(p) at p ~ 4096, would otherwise hide under level 0.  A
level whose reference is all zero (masked off, or nobody's gradient) must be torch.equal to its initial contents.  The twin sums
sequentially, so no atomic allowance is added; the fixed-point quantisation of the binned reduce (2^-40 of the level maximum per
record) needs no term of its own.  Every case runs first-order only (gE), with the second-order term (gE, gG, q) and with
gE = NULL (the double-backward route of tinycudann.py); cases with the second-order term use points re-drawn away from the
lattice planes (hash_bwd_refs.make_points).

The guard test comes first: a table with a level of more than 64 slices must be refused by the binned entry point before anything
is enqueued.  That configuration is never run through the binned kernels.

Out of scope: NaN gradients (only a +inf level is specified, test_binned_non_finite_level), n_features other than 2, the forward's
XCD-partitioned variant outside configuration A, timing.

Measured on the MI355X (err = max|got - ref64|, e32 = max|twin32 - ref64|; per path, term, configuration and group of cases the
level and case with the largest err/e32, as backward_refs.format_table() prints it when the module's fixture is torn down).  The
whole file runs in 29 s there (249 cases; the three 4 M-point cases take 3.8 s each, every other case under a second):

    quantity                                           err       e32  err/e32   worst case
    hash_bwd guard-cfg fields both                1.81e-02  1.80e-02     1.01   n=32773 level=7
    hash_bwd atomic first A rows                  1.95e-06  1.95e-06     1.00   n=4099 level=0
    hash_bwd atomic both A rows                   4.75e-04  3.67e-04     1.30   n=4099 level=2
    hash_bwd atomic second A rows                 4.83e-04  3.70e-04     1.30   n=4099 level=2
    hash_bwd binned first A rows                  2.01e-06  1.95e-06     1.03   n=4099 level=0
    hash_bwd binned both A rows                   4.75e-04  3.67e-04     1.30   n=4099 level=2
    hash_bwd binned second A rows                 4.83e-04  3.70e-04     1.30   n=4099 level=2
    hash_bwd atomic first odd5 rows               2.01e-06  1.95e-06     1.03   n=4099 level=0
    hash_bwd atomic both odd5 rows                4.75e-04  3.67e-04     1.30   n=4099 level=2
    hash_bwd atomic second odd5 rows              4.83e-04  3.70e-04     1.30   n=4099 level=2
    hash_bwd atomic first one rows                2.01e-06  1.95e-06     1.03   n=4099 level=0
    hash_bwd atomic both one rows                 3.57e-05  3.26e-05     1.09   n=129 level=0
    hash_bwd atomic second one rows               1.15e-04  1.03e-04     1.12   n=4099 level=0
    hash_bwd atomic first small12 rows            2.01e-06  1.95e-06     1.03   n=4099 level=0
    hash_bwd atomic both small12 rows             5.53e-04  4.40e-04     1.26   n=4099 level=2
    hash_bwd atomic second small12 rows           5.66e-04  4.31e-04     1.31   n=4099 level=2
    hash_bwd binned first odd5 rows               2.01e-06  1.95e-06     1.03   n=4099 level=0
    hash_bwd binned both odd5 rows                4.75e-04  3.67e-04     1.30   n=4099 level=2
    hash_bwd binned second odd5 rows              4.83e-04  3.70e-04     1.30   n=4099 level=2
    hash_bwd binned first one rows                2.01e-06  1.95e-06     1.03   n=4099 level=0
    hash_bwd binned both one rows                 1.11e-04  1.11e-04     1.00   n=4099 level=0
    hash_bwd binned second one rows               1.08e-04  1.03e-04     1.05   n=4099 level=0
    hash_bwd binned first small12 rows            2.01e-06  1.95e-06     1.03   n=4099 level=0
    hash_bwd binned both small12 rows             5.68e-04  4.40e-04     1.29   n=4099 level=2
    hash_bwd binned second small12 rows           5.66e-04  4.31e-04     1.31   n=4099 level=2
    hash_bwd atomic first A order                 1.80e-04  1.01e-04     1.78   pts=same level=3
    hash_bwd atomic both A order                  7.16e-03  5.20e-03     1.38   pts=alt2 level=3
    hash_bwd atomic second A order                4.83e-04  3.70e-04     1.30   pts=uniform level=2
    hash_bwd binned first A order                 1.88e-04  1.01e-04     1.85   pts=same level=3
    hash_bwd binned both A order                  4.75e-04  3.67e-04     1.30   pts=uniform level=2
    hash_bwd binned second A order                4.83e-04  3.70e-04     1.30   pts=uniform level=2
    hash_bwd atomic first A outside               1.26e-07  1.26e-07     1.00   pts=special level=0
    hash_bwd atomic both A outside                3.98e-03  3.97e-03     1.00   pts=special level=8
    hash_bwd atomic second A outside              3.97e-03  3.96e-03     1.00   pts=special level=8
    hash_bwd atomic first A far                   2.27e-05  2.27e-05     1.00   pts=far level=0
    hash_bwd atomic both A far                    8.09e-03  8.07e-03     1.00   pts=far level=3
    hash_bwd atomic second A far                  8.07e-03  8.06e-03     1.00   pts=far level=3
    hash_bwd atomic first odd5 outside            1.26e-07  1.26e-07     1.00   pts=special level=0
    hash_bwd atomic both odd5 outside             7.28e-06  7.28e-06     1.00   pts=special level=0
    hash_bwd atomic second odd5 outside           7.29e-06  7.29e-06     1.00   pts=special level=0
    hash_bwd atomic first odd5 far                2.27e-05  2.27e-05     1.00   pts=far level=0
    hash_bwd atomic both odd5 far                 8.09e-03  8.07e-03     1.00   pts=far level=3
    hash_bwd atomic second odd5 far               8.07e-03  8.06e-03     1.00   pts=far level=3
    hash_bwd atomic first one outside             1.26e-07  1.26e-07     1.00   pts=special level=0
    hash_bwd atomic both one outside              7.28e-06  7.28e-06     1.00   pts=special level=0
    hash_bwd atomic second one outside            7.29e-06  7.29e-06     1.00   pts=special level=0
    hash_bwd atomic first one far                 2.27e-05  2.27e-05     1.00   pts=far level=0
    hash_bwd atomic both one far                  6.81e-04  6.81e-04     1.00   pts=far level=0
    hash_bwd atomic second one far                6.63e-04  6.63e-04     1.00   pts=far level=0
    hash_bwd atomic first small12 outside         1.26e-07  1.26e-07     1.00   pts=special level=0
    hash_bwd atomic both small12 outside          4.40e-04  4.25e-04     1.04   pts=near level=2
    hash_bwd atomic second small12 outside        2.17e-03  2.15e-03     1.01   pts=near level=4
    hash_bwd atomic first small12 far             2.27e-05  2.27e-05     1.00   pts=far level=0
    hash_bwd atomic both small12 far              1.55e-03  1.46e-03     1.06   pts=far level=1
    hash_bwd atomic second small12 far            1.54e-03  1.46e-03     1.06   pts=far level=1
    hash_bwd binned first A outside               1.26e-07  1.26e-07     1.00   pts=special level=0
    hash_bwd binned both A outside                3.90e-02  3.89e-02     1.00   pts=near level=8
    hash_bwd binned second A outside              1.15e-04  1.10e-04     1.04   pts=near level=0
    hash_bwd binned first A far                   2.27e-05  2.27e-05     1.00   pts=far level=0
    hash_bwd binned both A far                    8.09e-03  8.07e-03     1.00   pts=far level=3
    hash_bwd binned second A far                  8.07e-03  8.06e-03     1.00   pts=far level=3
    hash_bwd binned first odd5 outside            1.26e-07  1.26e-07     1.00   pts=special level=0
    hash_bwd binned both odd5 outside             7.28e-06  7.28e-06     1.00   pts=special level=0
    hash_bwd binned second odd5 outside           1.15e-04  1.10e-04     1.04   pts=near level=0
    hash_bwd binned first odd5 far                2.27e-05  2.27e-05     1.00   pts=far level=0
    hash_bwd binned both odd5 far                 8.09e-03  8.07e-03     1.00   pts=far level=3
    hash_bwd binned second odd5 far               8.07e-03  8.06e-03     1.00   pts=far level=3
    hash_bwd binned first one outside             1.26e-07  1.26e-07     1.00   pts=special level=0
    hash_bwd binned both one outside              7.28e-06  7.28e-06     1.00   pts=special level=0
    hash_bwd binned second one outside            1.15e-04  1.10e-04     1.04   pts=near level=0
    hash_bwd binned first one far                 2.27e-05  2.27e-05     1.00   pts=far level=0
    hash_bwd binned both one far                  6.81e-04  6.81e-04     1.00   pts=far level=0
    hash_bwd binned second one far                6.63e-04  6.63e-04     1.00   pts=far level=0
    hash_bwd binned first small12 outside         1.26e-07  1.26e-07     1.00   pts=special level=0
    hash_bwd binned both small12 outside          4.33e-04  4.25e-04     1.02   pts=near level=2
    hash_bwd binned second small12 outside        1.15e-04  1.10e-04     1.04   pts=near level=0
    hash_bwd binned first small12 far             2.27e-05  2.27e-05     1.00   pts=far level=0
    hash_bwd binned both small12 far              1.55e-03  1.46e-03     1.06   pts=far level=1
    hash_bwd binned second small12 far            1.54e-03  1.46e-03     1.06   pts=far level=1
    hash_fwd enc A outside                        2.73e-07  2.65e-07     1.03   pts=near level=0
    hash_fwd dy_dx A outside                      2.33e-05  2.23e-05     1.04   pts=special level=3
    hash_fwd enc A far                            3.75e-05  3.75e-05     1.00   pts=far level=7
    hash_fwd dy_dx A far                          3.41e-03  3.41e-03     1.00   pts=far level=5
    hash_fwd enc odd5 outside                     2.73e-07  2.65e-07     1.03   pts=near level=0
    hash_fwd dy_dx odd5 outside                   2.33e-05  2.23e-05     1.04   pts=special level=3
    hash_fwd enc odd5 far                         2.98e-06  2.98e-06     1.00   pts=far level=0
    hash_fwd dy_dx odd5 far                       1.59e-04  1.59e-04     1.00   pts=far level=1
    hash_fwd enc one outside                      2.73e-07  2.65e-07     1.03   pts=near level=0
    hash_fwd dy_dx one outside                    2.02e-06  2.03e-06     1.00   pts=special level=0
    hash_fwd enc one far                          2.98e-06  2.98e-06     1.00   pts=far level=0
    hash_fwd dy_dx one far                        7.40e-05  7.40e-05     1.00   pts=far level=0
    hash_fwd enc small12 outside                  1.27e-07  1.19e-07     1.07   pts=special level=4
    hash_fwd dy_dx small12 outside                1.66e-04  1.66e-04     1.00   pts=special level=5
    hash_fwd enc small12 far                      8.38e-06  8.38e-06     1.00   pts=far level=2
    hash_fwd dy_dx small12 far                    7.40e-05  7.40e-05     1.00   pts=far level=0
    hash_bwd atomic first A views                 2.07e-06  1.95e-06     1.06   level=0
    hash_bwd atomic both A views                  4.75e-04  3.67e-04     1.30   level=2
    hash_bwd atomic second A views                4.83e-04  3.70e-04     1.30   level=2
    hash_bwd binned first A views                 2.01e-06  1.95e-06     1.03   level=0
    hash_bwd binned both A views                  4.75e-04  3.67e-04     1.30   level=2
    hash_bwd binned second A views                4.83e-04  3.70e-04     1.30   level=2
    hash_bwd atomic first A wave-skip             2.01e-06  1.95e-06     1.03   level=0
    hash_bwd atomic both A wave-skip              4.75e-04  3.67e-04     1.30   level=2
    hash_bwd atomic second A wave-skip            4.83e-04  3.70e-04     1.30   level=2
    hash_bwd binned first A masked                2.01e-06  1.95e-06     1.03   mask=0xfff level=0
    hash_bwd binned both A masked                 4.75e-04  3.67e-04     1.30   mask=0xfff level=2
    hash_bwd binned second A masked               4.83e-04  3.70e-04     1.30   mask=0xfff level=2
    hash_bwd binned first odd5 masked             2.01e-06  1.95e-06     1.03   mask=0xf level=0
    hash_bwd binned both odd5 masked              4.75e-04  3.67e-04     1.30   mask=0xf level=2
    hash_bwd binned second odd5 masked            4.83e-04  3.70e-04     1.30   mask=0xf level=2
    hash_bwd binned first A split                 8.21e-06  6.79e-06     1.21   n=70001 level=0
    hash_bwd binned both A split                  7.73e-04  7.43e-04     1.04   n=70001 level=2
    hash_bwd binned second A split                1.36e-02  1.35e-02     1.01   n=70001 level=6
    hash_bwd binned first one split               5.67e-05  2.63e-04     0.22   n=4194433 level=0
    hash_bwd binned both one split                2.34e-03  1.32e-02     0.18   n=4194433 level=0
    hash_bwd binned second one split              2.09e-03  1.05e-02     0.20   n=4194433 level=0
    hash_bwd binned first A exact-scratch         2.01e-06  1.95e-06     1.03   n=4099 level=0
    hash_bwd binned both A exact-scratch          4.75e-04  3.67e-04     1.30   n=4099 level=2
    hash_bwd binned second A exact-scratch        4.83e-04  3.70e-04     1.30   n=4099 level=2

Nothing needed more than the rule: the largest err/e32 stays below 2 (1.85 and 1.93 in two runs; all points identical, first
order: 4099 records per entry, summed as a wave tree by the kernels and one after the other by the twin; the atomic path's
figures move a little between runs).  The binned path lands BELOW the twin on the 4 M-point bucket (about 0.2): its sums are exact
integers, the twin's sequential fp32 sum of 8192 records per entry is not.

Mutations of csrc/hashgrid.hip this file was run against (each fails here; none of them can write out of bounds; counts out of the 237
cases the file had before the mask, skip and scratch cases ran with gE = NULL as well):
  sign of the z term of d w / d x flipped for odd corners   145 cases fail: every `both` / `second` case of both paths
  the e - e4 tail records of hash_reduce_kernel dropped     95 cases: the binned path from n = 63 on, masks, split buckets, scratch bounds
  a run merged across the round boundary of a unit          12 cases: binned `same` and `march` orders, small12 at n = 4099, split `one`
A fourth, `l + 1 <= n_levels` in the pair-load condition of hash_bin_unit_kernel, changes no value: the extra half of the 16-byte
load is the gradient of a level that does not exist and is never used; it only reads 8 bytes past the row.  No test can see it
short of reading past the end of an allocation, which this suite does not do on purpose.
"""
import functools

import pytest
import torch

from tests import backward_refs as BR
from tests import hash_bwd_refs as HR
from tests.backward_refs import compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
ALL = 0xFFFFFFFF
N_FULL = HR.N_FULL
PATHS = ("atomic", "binned")
ATOMIC_NS = (1, 63, 64, 65, 255, 256, 257, N_FULL)                      # wave and block edges, inactive tail lanes read row n - 1
BINNED_NS = (1, 63, 64, 65, 127, 128, 129, 511, 512, 513, N_FULL)       # round, unit (128 points) and workgroup (512) edges
SEED = {k: (s, g) for k, n, s, g in HR.POINT_SETS if n in (N_FULL, 8, 1000, 100)}


@pytest.fixture(scope="module", autouse=True)
def lib():
    from intrinsicavatar_amd import build
    build.build()
    from intrinsicavatar_amd import _lib as L
    n0 = len(BR.TABLE)
    yield L.lib()
    print("\n" + "\n".join("TABLE " + r for r in BR.format_table(BR.TABLE[n0:]).splitlines()))      # the docstring's table, of this run


def G(t):
    return None if t is None else t.to(DEV).contiguous()


@functools.lru_cache(maxsize=None)
def layout(name):
    return HR.layout(HR.cfg(name))


@functools.lru_cache(maxsize=None)
def problem(kind, n, seed, guard=16, n_levels=16):
    return HR.make_problem(kind, n, seed, guard, n_levels)


@functools.lru_cache(maxsize=12)          # (a pair of configuration A is 150 MB)
def reference(name, kind, n_total, mode, n):
    """(ref64, twin32) of the first n rows of a point set; computed once, shared, never written to"""
    seed, guard = SEED[kind]
    return HR.refs(problem(kind, n_total, seed, guard), mode, layout(name), n)


def cargs(c):
    return (c["n_levels"], 2, c["log2_hashmap_size"], c["base_resolution"], c["per_level_scale"])


def scratch_bytes(lib, c, n):
    return int(lib.ia_hashgrid_bwd_scratch_bytes(n, c["n_levels"], c["log2_hashmap_size"], c["base_resolution"], c["per_level_scale"]))


def table(lib, name, init=None):
    """a gradient table on the GPU: zeros, or a copy of `init`; its size is the library's own count as well as the reference's"""
    c, lay = HR.cfg(name), layout(name)
    assert int(lib.ia_hashgrid_n_entries(c["n_levels"], c["log2_hashmap_size"], c["base_resolution"], c["per_level_scale"])) == lay[0]
    return torch.zeros(lay[0] * 2, device=DEV) if init is None else init.to(DEV).clone()


@functools.lru_cache(maxsize=None)
def random_table(name):
    return torch.randn(layout(name)[0] * 2, generator=BR.seeded(77)) * 0.1


def call(lib, path, c, x, gE, gG, q, grad, mask=ALL, scratch=None, nb=None):
    """one backward through the C ABI; x, q, grad contiguous GPU tensors, gE / gG row-strided GPU views or None"""
    from intrinsicavatar_amd import _lib as L
    n = x.shape[0]
    pe, se = (L.base_ptr(gE), gE.stride(0)) if gE is not None else (None, 0)
    pg, sg = (L.base_ptr(gG), gG.stride(0)) if gG is not None else (None, 0)
    assert se % 2 == 0 and sg % 2 == 0                              # the header requires even strides
    assert grad.numel() == HR.layout(c)[0] * 2 and x.shape == (n, 3) and (q is None or q.shape == (n, 3))
    if path == "atomic":
        assert mask == ALL
        return lib.ia_hashgrid_bwd(n, x, *cargs(c), pe, se, pg, sg, q, grad)
    assert max(HR.n_slices(HR.layout(c))) <= 64, "a configuration the binned kernels must never see"
    if scratch is None:
        nb = scratch_bytes(lib, c, n)
        assert nb > 0
        scratch = torch.empty(nb, dtype=torch.uint8, device=DEV)
    return lib.ia_hashgrid_bwd_binned(n, x, *cargs(c), pe, se, pg, sg, q, grad, mask, L.ptr(scratch), nb)


def run(lib, path, name, inputs, init=None, mask=ALL):
    x, gE, gG, q = inputs
    grad = table(lib, name, init)
    call(lib, path, HR.cfg(name), G(x), G(gE), G(gG), G(q), grad, mask)
    return grad.cpu()


def check_levels(what, got, refs, lay, init=None, levels=None):
    """the comparison rule per level; an all-zero reference level must be torch.equal to its initial contents (zeros without init)"""
    r64, r32 = refs
    for l, sl in HR.level_slices(lay):
        if levels is not None and l not in levels:
            continue
        g = got[sl]
        if float(r64[sl].abs().max()) == 0.0:
            assert torch.equal(g, torch.zeros_like(g) if init is None else init[sl]), f"{what} level={l}: an untouched level changed"
        else:
            assert init is None
            compare(f"{what} level={l}", g, r64[sl], r32[sl])


def inputs_of(kind, n_total, mode, n, n_levels):
    seed, guard = SEED[kind]
    return HR.mode_inputs(problem(kind, n_total, seed, guard), mode, n, n_levels)


# ----------------------------------------------------------------------------------------------------------------------
# 0. the guard
def test_binned_refuses_a_level_of_more_than_64_slices(lib):
    """8 levels, 2^20 entries: 451 buckets pass the bucket-count check, levels 5..7 have 128 slices each, and the staged fill gives
    one lane and one UnitLds::cur entry to a slice.  The size query answers -1, the entry point returns a non-zero status with a
    sentinel-filled table and scratch untouched, and fields.hashgrid_backward takes the atomic path (method=None) or raises
    (method='binned').  The binned kernels are never launched on this configuration."""
    from intrinsicavatar_amd import _lib as L, fields
    c = HR.OVER_64_SLICES
    lay = HR.layout(c)
    n = HR.N_GUARD_CASE
    assert max(HR.n_slices(lay)) == 128 and sum(HR.n_slices(lay)) == 451
    assert int(lib.ia_hashgrid_n_entries(c["n_levels"], c["log2_hashmap_size"], c["base_resolution"], c["per_level_scale"])) == lay[0]
    assert scratch_bytes(lib, c, n) == -1                                   # (were it not, the call below would not be made)
    p = HR.make_problem("uniform", n, 20, "over64")
    x, gE, gG, q = (G(t) for t in HR.mode_inputs(p, "both", None, c["n_levels"]))
    grad = torch.full((lay[0] * 2,), 7.0, device=DEV)
    scratch = torch.full((64 << 20,), 0xA5, dtype=torch.uint8, device=DEV)
    rc = lib._cdll.ia_hashgrid_bwd_binned(n, x.data_ptr(), *cargs(c), gE.data_ptr(), gE.stride(0), gG.data_ptr(), gG.stride(0), q.data_ptr(),
                                          grad.data_ptr(), ALL, scratch.data_ptr(), scratch.numel(), L.stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert torch.equal(grad, torch.full_like(grad, 7.0)) and torch.equal(scratch, torch.full_like(scratch, 0xA5))
    del scratch
    with pytest.raises(L.IaError):
        fields.hashgrid_backward(x, gE, grad, cfg=c, g_jac=gG, q=q, method="binned")
    assert torch.equal(grad, torch.full_like(grad, 7.0))
    grad.zero_()
    fields.hashgrid_backward(x, gE, grad, cfg=c, g_jac=gG, q=q)              # n >= HASH_BWD_BINNED_MIN: the atomic path all the same
    assert n >= fields.HASH_BWD_BINNED_MIN
    check_levels(f"hash_bwd guard-cfg fields both n={n}", grad.cpu(), HR.refs(p, "both", lay), lay)


# ----------------------------------------------------------------------------------------------------------------------
# 1. row counts
ROW_CASES = [("atomic", "A", n) for n in ATOMIC_NS] + [("binned", "A", n) for n in BINNED_NS] + \
            [(path, name, n) for path in PATHS for name in ("odd5", "one", "small12") for n in (129, N_FULL)]


@pytest.mark.parametrize("mode", HR.MODES)
@pytest.mark.parametrize("path,name,n", ROW_CASES)
def test_row_counts(lib, path, name, n, mode):
    """the first n rows of the 4099-row uniform problem"""
    L_ = HR.cfg(name)["n_levels"]
    got = run(lib, path, name, inputs_of("uniform", N_FULL, mode, n, L_))
    check_levels(f"hash_bwd {path} {mode} {name} rows n={n}", got, reference(name, "uniform", N_FULL, mode, n), layout(name))


# ----------------------------------------------------------------------------------------------------------------------
# 2. point orders
@pytest.mark.parametrize("mode", HR.MODES)
@pytest.mark.parametrize("kind", ("uniform", "march", "same", "alt2"))
@pytest.mark.parametrize("path", PATHS)
def test_point_orders(lib, path, kind, mode):
    """uniform (no merging), marching order (run merging, the `heads != ~0` branch), all points identical (runs span whole waves
    and must not merge across the round boundary), two points alternating (no merging, one LDS address from every lane)"""
    got = run(lib, path, "A", inputs_of(kind, N_FULL, mode, N_FULL, 16))
    check_levels(f"hash_bwd {path} {mode} A order pts={kind}", got, reference("A", kind, N_FULL, mode, N_FULL), layout("A"))


# ----------------------------------------------------------------------------------------------------------------------
# 3. faces and outside
OUTSIDE = (("special", 8), ("near", 1000), ("far", 100))          # `far` in cases of its own: e32 = 6e-3 against 1e-4


@pytest.mark.parametrize("mode", HR.MODES)
@pytest.mark.parametrize("kind,n", OUTSIDE)
@pytest.mark.parametrize("name", tuple(HR.CONFIGS))
@pytest.mark.parametrize("path", PATHS)
def test_faces_and_outside(lib, path, name, kind, n, mode):
    L_ = HR.cfg(name)["n_levels"]
    got = run(lib, path, name, inputs_of(kind, n, mode, n, L_))
    check_levels(f"hash_bwd {path} {mode} {name} {'far' if kind == 'far' else 'outside'} pts={kind}", got, reference(name, kind, n, mode, n), layout(name))


@pytest.mark.parametrize("kind,n", OUTSIDE)
@pytest.mark.parametrize("name", tuple(HR.CONFIGS))
def test_forward_faces_and_outside(lib, name, kind, n):
    """ia_hashgrid_fwd (enc and dy_dx) on the same points against the forward reference: ties the reference's indices to the
    forward kernel, under all four configurations"""
    c, lay = HR.cfg(name), layout(name)
    L_ = c["n_levels"]
    seed, guard = SEED[kind]
    x = problem(kind, n, seed, guard)["x2"]                  # J jumps across a lattice plane: guarded points
    params = random_table(name)
    out = torch.full((n, 2 * L_), 1e3, device=DEV)
    jac = torch.full((n, 2 * L_, 3), 1e3, device=DEV)
    lib.ia_hashgrid_fwd(n, G(x), G(params), *cargs(c), out, 2 * L_, jac)
    e64, j64 = HR.forward(x, params, lay, F64)
    e32, j32 = HR.forward(x, params, lay, F32)
    out, jac = out.cpu(), jac.cpu()
    for l in range(L_):
        k = slice(2 * l, 2 * l + 2)
        compare(f"hash_fwd enc {name} {'far' if kind == 'far' else 'outside'} pts={kind} level={l}", out[:, k], e64[:, k], e32[:, k])
        compare(f"hash_fwd dy_dx {name} {'far' if kind == 'far' else 'outside'} pts={kind} level={l}", jac[:, k], j64[:, k], j32[:, k])


# ----------------------------------------------------------------------------------------------------------------------
# 4. strides and views
@pytest.mark.parametrize("mode", HR.MODES)
@pytest.mark.parametrize("path", PATHS)
def test_strides_and_views(lib, path, mode):
    """gE as columns 0..31 of a [n, 68] buffer (the radiance route), gG with stride 32, and every tensor a row slice that starts at
    row 128 of a larger buffer full of garbage"""
    n, lay, c = N_FULL, layout("A"), HR.cfg("A")
    x, gE, gG, q = inputs_of("uniform", N_FULL, mode, n, 16)

    def rows(t, cols, width):
        if t is None:
            return None
        big = torch.full((128 + n + 64, width), 1e3, device=DEV)
        big[128:128 + n, :cols] = t.to(DEV)
        return big[128:128 + n, :cols]
    xs, qs = rows(x, 3, 3), rows(q, 3, 3)
    ge, gg = rows(gE, 32, 68), rows(gG, 32, 32)
    assert ge is None or ge.stride(0) == 68
    big = torch.full((lay[0] * 2 + 512,), 7.0, device=DEV)
    grad = big[256:256 + lay[0] * 2]
    grad.zero_()
    nb = scratch_bytes(lib, c, n)
    sbuf = torch.empty(nb + 4096, dtype=torch.uint8, device=DEV)
    call(lib, path, c, xs, ge, gg, qs, grad, scratch=sbuf[1:1 + nb], nb=nb)
    got = big.cpu()
    assert bool((got[:256] == 7.0).all()) and bool((got[256 + lay[0] * 2:] == 7.0).all())
    check_levels(f"hash_bwd {path} {mode} A views", got[256:256 + lay[0] * 2], reference("A", "uniform", N_FULL, mode, n), lay)


# ----------------------------------------------------------------------------------------------------------------------
# 5. wave-level skip (atomic path)
@pytest.mark.parametrize("mode", HR.MODES)
def test_atomic_wave_level_skip(lib, mode):
    """level 3 of the gradients is zero in rows 0..63 only (the first wave skips the level, the others do not); level 7 is zero
    everywhere: its slice keeps its initial contents"""
    lay = layout("A")
    x, gE, gG, q = inputs_of("uniform", N_FULL, mode, N_FULL, 16)

    def cut(t):
        if t is None:
            return None
        t = t.clone()
        t[:64, 6:8] = 0.0
        t[:, 14:16] = 0.0
        return t
    gE, gG = cut(gE), cut(gG)
    refs = (HR.table_grad(x, gE, gG, q, lay, F64), HR.table_grad(x, gE, gG, q, lay, F32))
    assert float(refs[0][HR.level_slices(lay)[7][1]].abs().max()) == 0.0
    check_levels(f"hash_bwd atomic {mode} A wave-skip", run(lib, "atomic", "A", (x, gE, gG, q)), refs, lay)
    init = random_table("A")
    got = run(lib, "atomic", "A", (x, gE, gG, q), init=init)
    check_levels(f"hash_bwd atomic {mode} A wave-skip", got, refs, lay, init=init, levels=(7,))


# ----------------------------------------------------------------------------------------------------------------------
# 6. level mask (binned path)
MASK_CASES = [("A", m) for m in (0x0FFF, 0x5555, 0xAAAA, 0x0001, 0x8000)] + [("odd5", 0x10), ("odd5", 0x0F)]


@pytest.mark.parametrize("mode", HR.MODES)
@pytest.mark.parametrize("name,mask", MASK_CASES)
def test_binned_level_mask(lib, name, mask, mode):
    """gE and gG non-zero on every level; masked levels keep a random initial table bit for bit, unmasked levels follow the rule
    (into zeros) and are init + r bit for bit (into the random table: single-part buckets, plain read-modify-write).  Masks with
    half-on pairs; under odd5 0x10 enables the last level alone (the tail branch of the pair load)."""
    lay = layout(name)
    L_ = HR.cfg(name)["n_levels"]
    on = [l for l in range(L_) if (mask >> l) & 1]
    inputs = inputs_of("uniform", N_FULL, mode, N_FULL, L_)
    r64, r32 = reference(name, "uniform", N_FULL, mode, N_FULL)
    r = run(lib, "binned", name, inputs, mask=mask)
    init = random_table(name)
    got = run(lib, "binned", name, inputs, init=init, mask=mask)
    for l, sl in HR.level_slices(lay):
        if l in on:
            compare(f"hash_bwd binned {mode} {name} masked mask={mask:#x} level={l}", r[sl], r64[sl], r32[sl])
            assert torch.equal(got[sl], init[sl] + r[sl]), (name, hex(mask), l)
        else:
            assert torch.equal(r[sl], torch.zeros_like(r[sl])) and torch.equal(got[sl], init[sl]), (name, hex(mask), l)


# ----------------------------------------------------------------------------------------------------------------------
# 7. accumulation (binned path)
@pytest.mark.parametrize("mode", HR.MODES)
def test_binned_accumulation(lib, mode):
    """n = 4099: every bucket has a single part, so the reduce is a plain read-modify-write of exact integer sums: into a random
    table the result is init + r bit for bit (r: the same call into zeros), a second run is bit-identical, and entries that no
    record touches hold init exactly"""
    inputs = inputs_of("uniform", N_FULL, mode, N_FULL, 16)
    r = run(lib, "binned", "A", inputs)
    assert torch.equal(r, run(lib, "binned", "A", inputs))
    init = random_table("A")
    got = run(lib, "binned", "A", inputs, init=init)
    assert torch.equal(got, init + r)
    untouched = reference("A", "uniform", N_FULL, mode, N_FULL)[0] == 0
    assert int(untouched.sum()) > 0 and torch.equal(got[untouched], init[untouched])


# ----------------------------------------------------------------------------------------------------------------------
# 8. split buckets (binned path)
@pytest.mark.parametrize("mode", HR.MODES)
@pytest.mark.parametrize("name,n,seed,guard", (("A", HR.N_TWO_PARTS, 18, 16), ("one", HR.N_CLAMPED_PARTS, 19, 1)))
def test_binned_split_buckets(lib, name, n, seed, guard, mode):
    """level 0 of A at n = 70 001 has 560 008 records: two parts, float atomics into the table, the per / s / e arithmetic;
    `one` at n = 64 * 65 536 + 129 has more than MAX_PARTS * PART_RECORDS records in its one bucket: nparts is clamped"""
    lay = layout(name)
    L_ = HR.cfg(name)["n_levels"]
    p = problem("uniform", n, seed, guard, L_)
    got = run(lib, "binned", name, HR.mode_inputs(p, mode, None, L_))
    check_levels(f"hash_bwd binned {mode} {name} split n={n}", got, HR.refs(p, mode, lay), lay)
    if mode == "second":
        problem.cache_clear()              # (the 4 M-point problem is not needed again)


# ----------------------------------------------------------------------------------------------------------------------
# 9. scratch bounds (binned path)
@pytest.mark.parametrize("mode", HR.MODES)
@pytest.mark.parametrize("n", (129, N_FULL))
def test_binned_scratch_bounds(lib, n, mode):
    """the work area is exactly ia_hashgrid_bwd_scratch_bytes bytes at the least favourable address (1 past a multiple of 256: the
    pieces then end at its last byte) with 4 KiB of sentinel behind it; one byte less is refused with the table untouched"""
    from intrinsicavatar_amd import _lib as L
    c, lay = HR.cfg("A"), layout("A")
    x, gE, gG, q = (G(t) for t in inputs_of("uniform", N_FULL, mode, n, 16))
    nb = scratch_bytes(lib, c, n)
    buf = torch.full((1 + nb + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    grad = torch.full((lay[0] * 2,), 7.0, device=DEV)
    with pytest.raises(L.IaError):
        call(lib, "binned", c, x, gE, gG, q, grad, scratch=buf[1:nb], nb=nb - 1)
    torch.cuda.synchronize()
    assert torch.equal(grad, torch.full_like(grad, 7.0)) and bool((buf == 0xA5).all())
    grad.zero_()
    call(lib, "binned", c, x, gE, gG, q, grad, scratch=buf[1:1 + nb], nb=nb)
    assert bool((buf[1 + nb:] == 0xA5).all()) and int(buf[0]) == 0xA5
    check_levels(f"hash_bwd binned {mode} A exact-scratch n={n}", grad.cpu(), reference("A", "uniform", N_FULL, mode, n), lay)


# ----------------------------------------------------------------------------------------------------------------------
# 10. non-finite level (binned path)
@pytest.mark.parametrize("mode", ("first", "both"))
def test_binned_non_finite_level(lib, mode):
    """one +inf in gE at level 3 (so not with gE = NULL): that level's slice is left as it was, every other level is bit for bit
    the finite run's (single-part buckets).  NaN gradients are out of scope: include/ia_amd.h specifies the +-inf case only."""
    lay = layout("A")
    x, gE, gG, q = inputs_of("uniform", N_FULL, mode, N_FULL, 16)
    init = random_table("A")
    fin = run(lib, "binned", "A", (x, gE, gG, q), init=init)
    bad = gE.clone()
    bad[1234, 6] = float("inf")
    got = run(lib, "binned", "A", (x, bad, gG, q), init=init)
    for l, sl in HR.level_slices(lay):
        assert torch.equal(got[sl], init[sl] if l == 3 else fin[sl]), l
    assert not torch.equal(fin[HR.level_slices(lay)[3][1]], init[HR.level_slices(lay)[3][1]])
