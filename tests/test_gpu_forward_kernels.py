"""GPU: every forward field kernel ALONE -- ia_mlp_fwd (kinds 0, 1, 2), ia_sdf_levels_fwd_grad, the six selectable kernels of
ia_sdf_levels_fwd, ia_sh4_fwd -- on inputs of its own against an fp64 reference of the same operation, and the level-major layouts
of the hash gather against the flat kernel.

The field tests compare these kernels with the reference modules at rtol 2e-5 .. 2e-3 on one golden batch or a near-initial
network, and the value-head variants only with each other.  Here each kernel is called through the C entry point (so y_stride,
the segment strides and the work areas are the test's), at the row counts where its tiling, grid-stride loop and software
pipeline change path (tests/forward_refs.py derives them), with the product's `mul / add` on the xyz segment, in a Softplus
regime inside the knee and one saturated on both sides, and compared by the rule of tests/backward_refs.py:
max|got - ref64| <= max(16 * e32, 32 ulp of max|ref64|), e32 = the error of the same formula in fp32 on the CPU.  Cases below 257
rows are the first rows of the 257-row problem and take its e32 (forward_refs.compare_rows).  Every output buffer has one
sentinel row behind it; where y_stride exceeds the output width the extra columns hold sentinels that must survive.  Re-runs of
one kernel through another source layout, and the layouts the gather leaves, are compared with torch.equal.

Out of scope: ia_sdf_levels_fwd switches to the predecessor pipeline at n >= 2^28 points (the default kernel addresses a level
pair with a 32-bit offset); a batch of that size needs tens of GB, the switch is not exercised here.  IA_SDF_HEAD=probe_cached is
a diagnostic that gives wrong values by design.

Measured on the MI355X (err = max|got - ref64|, e32 = max|twin32 - ref64|; the largest err/e32 per kernel and quantity over all
cases of this file, as backward_refs.format_table() prints it for the rows of this module when its fixture is torn down):

    quantity                                           err       e32  err/e32   worst case
    mlp1 fwd y                                    4.13e-07  3.54e-07     1.17   n=63 ys=3
    mlp2 fwd y                                    4.84e-07  4.54e-07     1.07   n=385 ys=5
    mlp1 fwd zero-units y                         3.41e-07  3.85e-07     0.89   n=257
    mlp2 fwd zero-units y                         4.90e-07  3.71e-07     1.32   n=257
    mlp1 fwd saturated y                          5.54e-06  3.95e-06     1.40   n=257
    mlp2 fwd saturated y                          9.48e-06  9.54e-06     0.99   n=257
    sdf head narrow y                             4.20e-07  3.86e-07     1.09   n=98341 ys=13
    sdf head narrow y (with grad)                 4.20e-07  3.86e-07     1.09   n=98341 ys=13
    sdf head narrow grad                          1.03e-07  7.17e-08     1.44   n=385 ys=13
    sdf head wide y                               7.30e-07  7.30e-07     1.00   n=385 ys=13
    sdf head wide y (with grad)                   7.30e-07  7.30e-07     1.00   n=385 ys=13
    sdf head wide grad                            5.21e-07  4.32e-07     1.21   n=385 ys=13
    sdf levels narrow y                           4.20e-07  3.86e-07     1.09   n=98341 ys=13
    sdf levels narrow grad                        1.03e-07  7.17e-08     1.44   n=385 ys=13
    sdf levels wide y                             7.30e-07  7.30e-07     1.00   n=385 ys=13
    sdf levels wide grad                          5.21e-07  4.32e-07     1.21   n=385 ys=13
    sdf value default narrow                      1.46e-07  1.89e-07     0.77   n=131105
    sdf value pipe2w12 narrow                     1.46e-07  1.89e-07     0.77   n=131105
    sdf value pipe2w8 narrow                      1.46e-07  1.89e-07     0.77   n=131105
    sdf value pipe12 narrow                       1.29e-07  1.89e-07     0.68   n=131105
    sdf value pipe8 narrow                        1.29e-07  1.89e-07     0.68   n=131105
    sdf value tile narrow                         2.01e-07  1.89e-07     1.06   n=131105
    sdf value default wide                        5.47e-07  5.93e-07     0.92   n=262177
    sdf value pipe2w12 wide                       5.47e-07  5.93e-07     0.92   n=262177
    sdf value pipe2w8 wide                        5.47e-07  5.93e-07     0.92   n=262177
    sdf value pipe12 wide                         4.91e-07  5.93e-07     0.83   n=262177
    sdf value pipe8 wide                          4.91e-07  5.93e-07     0.83   n=262177
    sdf value tile wide                           3.94e-07  3.94e-07     1.00   n=33
    sh4 fwd                                       1.22e-07  1.22e-07     1.00   n=255 stride=16

No quantity needs more than 1.5 x e32: the value head's Softplus without the threshold pass-through, its weights pre-scaled by
100 log2(e), and log1p taken as log(1 + e) all stay inside what a straightforward fp32 evaluation loses, in both regimes.  The
whole file takes 6 s (125 cases, the slowest 1 s: the four source layouts of kind 1 at 98 341 rows).
"""
import ctypes as C
import functools

import pytest
import torch

from tests import backward_refs as BR
from tests import forward_refs as FR
from tests.forward_refs import compare_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.0


@pytest.fixture(scope="module", autouse=True)
def lib():
    from intrinsicavatar_amd import build
    build.build()
    from intrinsicavatar_amd import _lib as L
    first = len(BR.TABLE)                    # the rows of this module only, not the whole process's
    yield L.lib()
    print("\n" + "\n".join("TABLE " + r for r in BR.format_table(BR.TABLE[first:]).splitlines()))


def G(t):
    return None if t is None else t.to(DEV).contiguous()


def guarded(n, cols):
    """an [n, cols] output buffer, sentinel-filled, with one sentinel row behind it: (whole buffer, the n rows)."""
    full = torch.full((n + 1, cols), SENTINEL, device=DEV)
    return full, full[:n]


def check_guard(what, full, width=None):
    """nothing behind the last row was written, nor any column >= width of the rows themselves."""
    assert bool((full[-1] == SENTINEL).all()), f"{what}: the kernel wrote behind the last row"
    if width is not None and width < full.shape[1]:
        assert bool((full[:-1, width:] == SENTINEL).all()), f"{what}: the kernel wrote into the columns beyond the output width"


def floats(*v):
    return (C.c_float * len(v))(*[float(x) for x in v])


# ----------------------------------------------------------------------------------------------------------------------
# A. ia_mlp_fwd kinds 1 and 2
def mlp2_segments(kind, segs, layout, n):
    """device tensors of the segments in one of four source layouts -> [(tensor, width, mul, add)] for _lib.segments."""
    spec = BR.MLP2_SPEC[kind]
    if layout == "contiguous":
        ts = [G(s) for s in segs]
    elif layout == "offset1":                 # every segment a view at storage offset 1: no 16-byte alignment, the scalar path
        ts = []
        for s, (w, _, _) in zip(segs, spec):
            flat = torch.full((n * w + 1,), SENTINEL, device=DEV)
            flat[1:] = G(s).reshape(-1)
            ts.append(flat[1:].view(n, w))
            assert ts[-1].data_ptr() % 16 == 4
    elif layout == "column48":                # segment 0 a column view of an aligned [n,48] buffer: the vector path, stride != width
        buf = torch.full((n, 48), SENTINEL, device=DEV)
        buf[:, :32] = G(segs[0])
        ts = [buf[:, :32]] + [G(s) for s in segs[1:]]
        assert ts[0].data_ptr() % 16 == 0 and ts[0].stride(0) == 48
    else:                                     # "row71": all segments views of one [n,71] row from column 1 on
        buf = torch.full((n, 71), SENTINEL, device=DEV)
        ts, c = [], 1
        for s, (w, _, _) in zip(segs, spec):
            buf[:, c:c + w] = G(s)
            ts.append(buf[:, c:c + w])
            c += w
    return [(t, w, m, a) for t, (w, m, a) in zip(ts, spec)]


def run_mlp2(lib, kind, p, n, y_stride, layout="contiguous"):
    from intrinsicavatar_amd import _lib as L
    OUT = BR.MLP2_OUT[kind]
    segs = mlp2_segments(kind, [s[:n] for s in p["segs"]], layout, n)
    ws = [G(w) for w in p["weights"]]
    full, y = guarded(n, y_stride)
    lib.ia_mlp_fwd(kind, n, *L.segments(segs), *ws, full, y_stride, None, 0, None, None)
    check_guard(f"mlp{kind} fwd n={n} ys={y_stride} {layout}", full, OUT)
    return y[:, :OUT]


@pytest.mark.parametrize("n", FR.MLP_NS)
@pytest.mark.parametrize("kind", [1, 2])
def test_mlp2_forward(lib, kind, n):
    """ia_mlp_fwd kinds 1 / 2 with the product's segment spec (xyz times 2 minus 1): y by the rule with y_stride = OUT and OUT + 3;
    at n = 33 and 98 341 three more source layouts (scalar assembly at storage offset 1, the 16-byte path through a row stride
    of 48, column views of one 71-wide row) give the bits of the contiguous run."""
    OUT = BR.MLP2_OUT[kind]
    p, r64, t32 = FR.mlp2_case(kind, FR.problem_rows(n))
    ys = {}
    for y_stride in (OUT, OUT + 3):
        ys[y_stride] = run_mlp2(lib, kind, p, n, y_stride)
        compare_rows(f"mlp{kind} fwd y n={n} ys={y_stride}", ys[y_stride], r64["y"], t32["y"])
    assert torch.equal(ys[OUT], ys[OUT + 3])
    if n in FR.MLP_LAYOUT_NS:
        for layout in ("offset1", "column48", "row71"):
            assert torch.equal(run_mlp2(lib, kind, p, n, OUT, layout), ys[OUT]), layout


@pytest.mark.parametrize("kind", [1, 2])
def test_mlp2_forward_exact_zero_preactivations(lib, kind):
    """a unit of each hidden layer whose pre-activation is exactly 0 in every row (backward_refs.MLP2_ZERO_CASE)."""
    n, seed = BR.MLP2_ZERO_CASE
    p, r64, t32 = FR.mlp2_case(kind, n, seed, zero_units=True)
    compare_rows(f"mlp{kind} fwd zero-units y n={n}", run_mlp2(lib, kind, p, n, BR.MLP2_OUT[kind]), r64["y"], t32["y"])


@pytest.mark.parametrize("kind", [1, 2])
def test_mlp2_forward_saturated_sigmoid(lib, kind):
    """Wo and bo times 40: a fifth and more of the outputs beyond |z3| = 30 on either side (up to 330): the sigmoid's __expf
    overflows to inf there and the result must still be finite (compare_rows asserts it) and by the rule."""
    n, seed = FR.SATURATED_CASE
    p, r64, t32 = FR.mlp2_case(kind, n, seed, saturated=True)
    y = run_mlp2(lib, kind, p, n, BR.MLP2_OUT[kind])
    compare_rows(f"mlp{kind} fwd saturated y n={n}", y, r64["y"], t32["y"])
    assert bool(((y >= 0) & (y <= 1)).all())


# ----------------------------------------------------------------------------------------------------------------------
# B. ia_mlp_fwd kind 0, C. ia_sdf_levels_fwd_grad
@functools.lru_cache(maxsize=4)
def sdf_head_inputs(n, regime):
    """the first n rows of the case's problem on the device, row-major."""
    p, r64, t32 = FR.sdf_head_case(FR.problem_rows(n), regime)
    dev = dict(enc=G(p["enc"][:n]), x=G(p["x"][:n]), jac=G(p["jac"][:n]), ws=[G(p[k]) for k in ("W1", "b1", "W2", "b2")])
    return dev, r64, t32


def run_sdf_head(lib, d, n, y_stride, with_grad):
    from intrinsicavatar_amd import _lib as L
    W1, b1, W2, b2 = d["ws"]
    fy, y = guarded(n, y_stride)
    fg, grad = guarded(n, 3)
    segs = L.segments([(d["enc"], 32, 1.0, 0.0), (d["x"], 3, 2.0, -1.0)])
    if with_grad:
        lib.ia_mlp_fwd(0, n, *segs, W1, b1, None, None, W2, b2, fy, y_stride, d["jac"], 32, floats(*FR.inv_scale()), fg)
    else:
        lib.ia_mlp_fwd(0, n, *segs, W1, b1, None, None, W2, b2, fy, y_stride, None, 0, None, None)
    check_guard(f"sdf head n={n} ys={y_stride} grad={int(with_grad)} y", fy, 13)
    check_guard(f"sdf head n={n} ys={y_stride} grad={int(with_grad)} grad", fg)
    if not with_grad:
        assert bool((fg == SENTINEL).all())
    return y[:, :13], grad


@pytest.mark.parametrize("n,regime", FR.sdf_head_cases())
def test_sdf_head_forward(lib, n, regime):
    """ia_mlp_fwd kind 0 on row-major sources: without the gradient y [13] by the rule (y_stride 13 and 16); with it (jac [n,32,3],
    xyz_col 32, inv_scale = 1 / extent of a non-uniform box) y and grad by the rule as separate quantities, y bit-equal to the
    run without."""
    d, r64, t32 = sdf_head_inputs(n, regime)
    tag = f"sdf head {regime}"
    for y_stride in (13, 16):
        y0, _ = run_sdf_head(lib, d, n, y_stride, False)
        compare_rows(f"{tag} y n={n} ys={y_stride}", y0, r64["out"], t32["out"])
        y1, grad = run_sdf_head(lib, d, n, y_stride, True)
        compare_rows(f"{tag} y (with grad) n={n} ys={y_stride}", y1, r64["out"], t32["out"])
        compare_rows(f"{tag} grad n={n} ys={y_stride}", grad, r64["grad"], t32["grad"])
        assert torch.equal(y0, y1)


def test_sdf_head_gradient_without_a_jacobian_is_refused(lib):
    """grad given, jac NULL: an error from the binding, nothing is launched (the output buffers keep their sentinels)."""
    from intrinsicavatar_amd import _lib as L
    n = 33
    d, _, _ = sdf_head_inputs(n, "narrow")
    W1, b1, W2, b2 = d["ws"]
    fy, _ = guarded(n, 13)
    fg, _ = guarded(n, 3)
    segs = L.segments([(d["enc"], 32, 1.0, 0.0), (d["x"], 3, 2.0, -1.0)])
    with pytest.raises(L.IaError):
        lib.ia_mlp_fwd(0, n, *segs, W1, b1, None, None, W2, b2, fy, 13, None, 32, floats(*FR.inv_scale()), fg)
    torch.cuda.synchronize()
    assert bool((fy == SENTINEL).all()) and bool((fg == SENTINEL).all())


def run_sdf_levels_grad(lib, d, n, y_stride):
    W1, b1, W2, b2 = d["ws"]
    levels, levels_jac = FR.to_levels(d["enc"]), FR.to_levels_jac(d["jac"])         # two separate tensors
    fy, y = guarded(n, y_stride)
    fg, grad = guarded(n, 3)
    lib.ia_sdf_levels_fwd_grad(n, levels, levels_jac, d["x"], W1, b1, W2, b2, fy, y_stride, floats(*FR.inv_scale()), fg)
    check_guard(f"sdf levels n={n} ys={y_stride} y", fy, 13)
    check_guard(f"sdf levels n={n} ys={y_stride} grad", fg)
    return y[:, :13], grad


@pytest.mark.parametrize("n,regime", FR.sdf_head_cases())
def test_sdf_head_forward_on_level_major_sources(lib, n, regime):
    """ia_sdf_levels_fwd_grad: the problems of test_sdf_head_forward handed over as float2 [16][n] and float [16][n][6]
    (forward_refs.to_levels / to_levels_jac), y_stride 13 and 16: y and grad by the rule."""
    d, r64, t32 = sdf_head_inputs(n, regime)
    tag = f"sdf levels {regime}"
    for y_stride in (13, 16):
        y, grad = run_sdf_levels_grad(lib, d, n, y_stride)
        compare_rows(f"{tag} y n={n} ys={y_stride}", y, r64["out"], t32["out"])
        compare_rows(f"{tag} grad n={n} ys={y_stride}", grad, r64["grad"], t32["grad"])


def test_sdf_levels_grad_refuses_a_short_row_stride(lib):
    from intrinsicavatar_amd import _lib as L
    n = 33
    d, _, _ = sdf_head_inputs(n, "narrow")
    W1, b1, W2, b2 = d["ws"]
    fy, _ = guarded(n, 13)
    fg, _ = guarded(n, 3)
    with pytest.raises(L.IaError):
        lib.ia_sdf_levels_fwd_grad(n, FR.to_levels(d["enc"]), FR.to_levels_jac(d["jac"]), d["x"], W1, b1, W2, b2, fy, 12,
                                   floats(*FR.inv_scale()), fg)
    torch.cuda.synchronize()
    assert bool((fy == SENTINEL).all()) and bool((fg == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------------------
# D. ia_sdf_levels_fwd, every selectable kernel
@functools.lru_cache(maxsize=2)
def sdf_value_inputs(n, regime):
    """one fp64 reference per (n, regime) for all six kernels; the first n rows on the device, features level-major."""
    p, r64, t32 = FR.sdf_value_case(FR.problem_rows(n), regime)
    dev = dict(levels=FR.to_levels(G(p["enc"][:n])), x=G(p["x"][:n]), ws=[G(p[k]) for k in ("W1", "b1", "W2", "b2")])
    return dev, r64, t32


@pytest.mark.parametrize("kernel", FR.VALUE_KERNELS, ids=lambda k: k or "default")
@pytest.mark.parametrize("n,regime", FR.sdf_value_cases())
def test_sdf_value_head(lib, monkeypatch, n, regime, kernel):
    """ia_sdf_levels_fwd, the kernel chosen through IA_SDF_HEAD (read on every call): sdf against out[:,0] of the fp64 head by the
    rule; n = k * 131 072 + 33 gives the waves of the default kernel k and k + 1 tiles (1 .. 5) and a one-row last tile.  The
    float behind sdf[n-1] is a sentinel."""
    if kernel is None:
        monkeypatch.delenv("IA_SDF_HEAD", raising=False)
    else:
        monkeypatch.setenv("IA_SDF_HEAD", kernel)
    d, r64, t32 = sdf_value_inputs(n, regime)
    W1, b1, W2, b2 = d["ws"]
    full = torch.full((n + 1,), SENTINEL, device=DEV)
    lib.ia_sdf_levels_fwd(n, d["levels"], d["x"], W1, b1, W2, b2, full)
    assert float(full[n]) == SENTINEL, "the kernel wrote behind sdf[n-1]"
    compare_rows(f"sdf value {kernel or 'default'} {regime} n={n}", full[:n], r64, t32)


# ----------------------------------------------------------------------------------------------------------------------
# E. ia_sh4_fwd
@pytest.mark.parametrize("n", FR.SH_NS)
def test_sh4_forward(lib, n):
    """ia_sh4_fwd on unit directions (the six axis directions and the diagonal first): into a contiguous [n,16], and into columns
    48..63 of a sentinel-filled [n,67] (out_stride 67) whose other columns must survive; the same bits both ways."""
    p, r64, t32 = FR.sh_case(FR.problem_rows(n))
    d01 = G(p["d01"][:n])
    full, out = guarded(n, 16)
    lib.ia_sh4_fwd(n, d01, full, 16)
    check_guard(f"sh4 n={n}", full)
    compare_rows(f"sh4 fwd n={n} stride=16", out, r64, t32)
    wide = torch.full((n + 1, 67), SENTINEL, device=DEV)
    lib.ia_sh4_fwd(n, d01, C.c_void_p(wide.data_ptr() + 48 * 4), 67)
    compare_rows(f"sh4 fwd n={n} stride=67", wide[:n, 48:64], r64, t32)
    assert torch.equal(wide[:n, 48:64], out)
    assert bool((wide[:, :48] == SENTINEL).all()) and bool((wide[:, 64:] == SENTINEL).all()) and bool((wide[n] == SENTINEL).all())


def test_sh4_refuses_a_short_row_stride(lib):
    from intrinsicavatar_amd import _lib as L
    p, _, _ = FR.sh_case(FR.PREFIX_ROWS)
    full, _ = guarded(33, 16)
    with pytest.raises(L.IaError):
        lib.ia_sh4_fwd(33, G(p["d01"][:33]), full, 15)
    torch.cuda.synchronize()
    assert bool((full == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------------------
# F. the layouts the gather leaves for the level-major heads
def test_level_major_gather_leaves_the_documented_layouts(lib):
    """ia_hashgrid_fwd_levels(with_jac = 1) into a work area of ia_hashgrid_fwd_scratch_bytes(n, 16, 1) bytes: the features at
    offset 0 are float2 [16][n], the Jacobian at ia_hashgrid_fwd_levels_jac_offset(n, 16) is float [16][n][6] -- both torch.equal
    to forward_refs.to_levels / to_levels_jac of what the flat ia_hashgrid_fwd writes for the same points and table (the row-major
    outputs of this path are a transposing copy of that data and are pinned bit for bit to the flat kernel elsewhere, so equality
    is a property, not a tolerance).  With sections C and D this fixes the layouts from both sides: writer and readers."""
    from intrinsicavatar_amd import fields
    cfg = fields.HASH
    n = fields.HASH_FWD_XCD_MIN + 37
    x = G(FR.make_hash_points(n))
    table = ((torch.rand(fields.hash_n_entries() * 2, generator=BR.seeded(11)) * 2.0 - 1.0) * 0.1).to(DEV)
    cargs = (cfg["n_levels"], cfg["n_features_per_level"], cfg["log2_hashmap_size"], cfg["base_resolution"], cfg["per_level_scale"])
    enc = torch.empty((n, 32), device=DEV)
    jac = torch.empty((n, 32, 3), device=DEV)
    lib.ia_hashgrid_fwd(n, x, table, *cargs, enc, 32, jac)
    nb = int(lib.ia_hashgrid_fwd_scratch_bytes(n, 16, 1))
    joff = int(lib.ia_hashgrid_fwd_levels_jac_offset(n, 16))
    assert joff >= 16 * n * 8 and joff % 4 == 0 and joff + 16 * n * 6 * 4 <= nb
    work = torch.full((nb + 256,), 0xA5, dtype=torch.uint8, device=DEV)              # 256 guard bytes behind the work area
    lib.ia_hashgrid_fwd_levels(n, x, table, *cargs, 1, work)
    assert bool((work[nb:] == 0xA5).all()), "the gather wrote behind its work area"
    levels = work[:16 * n * 8].view(torch.float32).view(16, n, 2)
    levels_jac = work[joff:joff + 16 * n * 6 * 4].view(torch.float32).view(16, n, 6)
    assert float(enc.abs().max()) > 0 and float(jac.abs().max()) > 0
    assert torch.equal(levels, FR.to_levels(enc))
    assert torch.equal(levels_jac, FR.to_levels_jac(jac))
