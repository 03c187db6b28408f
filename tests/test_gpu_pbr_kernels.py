"""GPU: the PBR shading kernels of csrc/pbr.hip per edge class -- forward of all four estimators, the one backward kernel
(pbr_light_bwd_kernel<0|1>) through its three callers, and every accumulator of the environment-image gradient -- against the plain
fp64 references of tests/pbr_refs.py.

The inputs are BUILT per edge class (tests/pbr_refs.py: last partial block, cosine-masked rows with NoL < 0 and NoL == 0, back-facing
views, tr in {0, 1, -0.1, 1.1}, roughness 0.05 and 1, metallic 0 and 1, albedo channels 0 and 1, the u = 0/1 seam, both clamped pole
rows, zero-pmf light texels, with and without indirect radiance), so that fp32, fp64 and the device take the same discrete decisions
for every sample: NO sample is excluded from any comparison.  Everything is compared by the rule of tests/backward_refs.py,
max|got - ref64| <= max(16 e32, 32 ulp of max|ref64|) with e32 = the error of the same formula in fp32 on the CPU, over ALL elements;
float-atomic sums carry that module's derived random-walk allowance with P = the largest number of adds one texel channel receives,
counted from the reference's indices; the 64-bit fixed-point path carries none.  Per-point quantities are compared per roughness
class (three comparisons that together cover every row): at roughness 0.05 the GGX lobe and its derivatives reach 1e2 .. 1e5 near
NoH = 1, and in one max-norm the fp32 error of those few rows would be the tolerance of all others.  Rows of masked classes are also
checked for exact zeros.

Measured on the MI355X (the largest err / e32 per quantity over all cases, as backward_refs.format_table() prints it at teardown):

    quantity                                           err       e32  err/e32   worst case
    shade light Lo                                4.08e-07  2.34e-07     1.74   F=256 map=5x7 ind=0 rough=lo
    shade light Lo_diff                           1.48e-06  7.43e-07     2.00   F=256 map=5x7 ind=1 rough=one
    shade light Lo_spec                           2.81e-08  3.37e-09     8.35   F=1 map=5x7 ind=1 rough=mid
    shade uniform_light Lo                        5.00e-08  3.94e-08     1.27   F=1 map=5x7 ind=1 rough=mid
    shade uniform_light Lo_diff                   4.69e-06  3.61e-06     1.30   F=256 map=16x32 ind=1 rough=lo
    shade uniform_light Lo_spec                   2.61e-08  2.16e-09    12.09   F=1 map=5x7 ind=1 rough=mid
    shade mis Lo                                  6.30e-07  2.88e-07     2.19   F=255 map=5x7 ind=1 rough=mid
    shade mis Lo_diff                             6.78e-07  4.58e-07     1.48   F=257 map=5x7 ind=0 rough=lo
    shade mis Lo_spec                             1.23e-08  2.43e-09     5.09   F=1 map=5x7 ind=0 rough=mid
    shade mats Lo                                 9.49e-07  2.88e-07     3.30   F=255 map=5x7 ind=1 rough=mid
    shade mats Lo_diff                            6.78e-07  4.72e-07     1.44   F=257 map=5x7 ind=0 rough=lo
    shade mats Lo_spec                            5.34e-08  6.17e-09     8.67   F=1 map=5x7 ind=1 rough=mid
    bwd light g_normal                            5.08e-06  6.64e-07     7.66   F=256 map=5x7 ind=0 from=Lo rough=mid
    bwd light g_albedo                            1.74e-06  3.97e-07     4.38   F=256 map=5x7 ind=0 from=Lo_spec rough=mid
    bwd light g_roughness                         1.05e-07  1.45e-08     7.24   F=1 map=16x32 ind=1 from=all rough=mid
    bwd light g_metallic                          9.37e-08  3.41e-08     2.75   F=1 map=5x7 ind=0 from=Lo rough=mid
    bwd light g_env direct                        3.00e-07  1.38e-07     2.18   F=1 map=5x7 ind=0 from=all
    bwd uniform_light g_normal                    6.55e-06  8.29e-07     7.90   F=256 map=5x7 ind=0 from=Lo rough=mid
    bwd uniform_light g_albedo                    1.97e-06  3.63e-07     5.42   F=256 map=5x7 ind=0 from=Lo_spec rough=mid
    bwd uniform_light g_roughness                 6.85e-06  2.32e-06     2.95   F=256 map=16x32 ind=1 from=Lo rough=one
    bwd uniform_light g_metallic                  3.52e-06  6.33e-07     5.55   F=257 map=16x32 ind=1 from=Lo_spec rough=mid
    bwd uniform_light g_env direct                5.11e-06  2.85e-06     1.80   F=256 map=5x7 ind=0 from=all
    bwd light (direct) g_normal                   1.55e-03  1.18e-03     1.32   F=262143 map=24x512 rough=one
    bwd light (direct) g_albedo                   4.17e-05  3.37e-05     1.24   F=257 map=24x512 rough=lo
    bwd light (direct) g_roughness                1.35e-05  5.38e-06     2.50   F=257 map=24x512 rough=one
    bwd light (direct) g_metallic                 5.33e-05  4.49e-05     1.19   F=257 map=24x512 rough=mid
    bwd uniform_light (direct) g_normal           1.17e-03  1.07e-03     1.10   F=257 map=24x512 rough=mid
    bwd uniform_light (direct) g_albedo           6.36e-05  5.59e-05     1.14   F=257 map=24x512 rough=mid
    bwd uniform_light (direct) g_roughness        8.12e-05  5.00e-05     1.62   F=257 map=24x512 rough=mid
    bwd uniform_light (direct) g_metallic         5.23e-05  5.23e-05     1.00   F=257 map=24x512 rough=one
    bwd light g_env fixed                         3.28e-03  4.94e-03     0.66   F=262144 map=24x512
    bwd light (fixed) g_normal                    5.11e-02  3.37e-02     1.51   F=262144 map=24x512 rough=lo
    bwd light (fixed) g_albedo                    6.83e-04  6.50e-04     1.05   F=262144 map=24x512 rough=one
    bwd light (fixed) g_roughness                 6.09e-03  4.83e-03     1.26   F=262144 map=24x512 rough=lo
    bwd light (fixed) g_metallic                  6.61e-04  6.12e-04     1.08   F=262144 map=24x512 rough=one
    bwd uniform_light g_env fixed                 2.81e-03  4.44e-03     0.63   F=270337 map=24x512
    bwd uniform_light (fixed) g_normal            3.75e-03  3.58e-03     1.05   F=270337 map=24x512 rough=mid
    bwd uniform_light (fixed) g_albedo            4.71e-04  6.95e-04     0.68   F=270337 map=24x512 rough=one
    bwd uniform_light (fixed) g_roughness         4.72e-04  5.16e-04     0.92   F=270337 map=24x512 rough=mid
    bwd uniform_light (fixed) g_metallic          4.29e-04  4.56e-04     0.94   F=270337 map=24x512 rough=one
    bwd uniform_light g_env unbinned              3.42e-03  4.52e-03     0.76   F=262144 map=24x512
    bwd uniform_light (unbinned) g_normal         6.07e-03  5.62e-03     1.08   F=262144 map=24x512 rough=mid
    bwd uniform_light (unbinned) g_albedo         4.29e-04  6.48e-04     0.66   F=262144 map=24x512 rough=mid
    bwd uniform_light (unbinned) g_roughness      6.27e-03  8.79e-03     0.71   F=262144 map=24x512 rough=lo
    bwd uniform_light (unbinned) g_metallic       3.53e-04  4.12e-04     0.86   F=262144 map=24x512 rough=one
    bwd light g_env unbinned                      3.60e-03  5.45e-03     0.66   F=270337 map=24x512
    bwd light (unbinned) g_normal                 3.42e-02  3.19e-02     1.07   F=270337 map=24x512 rough=lo
    bwd light (unbinned) g_albedo                 7.92e-04  6.63e-04     1.19   F=270337 map=24x512 rough=mid
    bwd light (unbinned) g_roughness              7.21e-03  6.84e-03     1.05   F=270337 map=24x512 rough=lo
    bwd light (unbinned) g_metallic               4.58e-04  4.75e-04     0.96   F=270337 map=24x512 rough=one
    scatterer lobes1 diff                         1.81e-08  3.16e-09     5.72   n=1 rough=mid
    scatterer lobes1 g_normal                     6.15e-08  3.79e-08     1.62   n=257 rough=mid
    scatterer lobes2 spec                         1.22e-09  1.22e-09     1.00   n=1 rough=mid
    scatterer lobes2 g_normal                     1.89e-06  1.36e-06     1.40   n=257 rough=mid
    scatterer lobes2 g_roughness                  9.90e-10  5.24e-10     1.89   n=1 rough=mid
    scatterer lobes2 g_albedo                     4.77e-09  1.04e-09     4.57   n=1 rough=mid
    scatterer lobes2 g_metallic                   4.23e-10  1.90e-10     2.23   n=1 rough=mid
    scatterer lobes3 diff                         1.81e-08  3.16e-09     5.72   n=1 rough=mid
    scatterer lobes3 spec                         1.22e-09  1.22e-09     1.00   n=1 rough=mid
    scatterer lobes3 g_normal                     1.87e-06  1.34e-06     1.40   n=257 rough=mid
    scatterer lobes3 g_roughness                  9.90e-10  5.24e-10     1.89   n=1 rough=mid
    scatterer lobes3 g_albedo                     4.77e-09  1.04e-09     4.57   n=1 rough=mid
    scatterer lobes3 g_metallic                   4.23e-10  1.90e-10     2.23   n=1 rough=mid

Nothing failed and nothing needed an exception: the largest ratio is 12 (a single-row case whose fp32 twin happens to round well).  The
e32 of the 512-wide maps (1e-5 .. 3e-4 of the result) is the fp32 formula's own loss: fx = u W - 1/2 near 256 has an ulp of 3e-5 texel,
and acos next to the poles turns the rounding of the direction into up to 0.007 texel rows.  The float-atomic texel sums move from run
to run; the fixed-point ones do not.

Sensitivity, each as a one-line change to a scratch copy of pbr.hip, run on the MI355X against this module: dropping `gNoV * wi` from
g_normal fails 20 of the 38 tests; dropping `(1 - met)` from gld 16; `ax` for `ay` in rec_w 5 (every record-path test); dropping bit 31 of
rec_idx 5; `x0 + 1` without the wrap in the binned accumulator 3 (the fixed-point tests); no tr clamp in the backward 16; ignoring g_Lo_spec
20.  Three more that the earlier guards of this kernel (test_pbr_shade_backward_vs_autograd, test_scatterer_eval_is_differentiable and the
banded-accumulation test) let pass or see only through another path: weight 0 instead of 1 at a zero-pmf texel in the backward fails 8,
the specular derivative left on for back-facing views 16, the bottom row's y1 clamped one row short in env_footprint 14.
"""
import functools

import pytest
import torch

from tests import backward_refs as BR
from tests import pbr_refs as PR
from tests.backward_refs import compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
BIG = 1 << 18                     # the threshold between the direct atomics and the record paths (ENV_ACC_MIN_F)
BIG_RAGGED = BIG + 8192 + 1       # a ragged last ENV_TILE; `per` of the unbinned kernel no multiple of 8 * 1024
FS = (1, 255, 256, 257)
SUBSETS = {"Lo": (True, False, False), "Lo_diff": (False, True, False), "Lo_spec": (False, False, True), "all": (True, True, True)}
POINT_GRADS = ("g_normal", "g_albedo", "g_roughness", "g_metallic")


@pytest.fixture(scope="module", autouse=True)
def lib():
    from intrinsicavatar_amd import build
    build.build()
    from intrinsicavatar_amd import _lib as L
    yield L.lib()
    print("\n" + "\n".join("TABLE " + r for r in BR.format_table().splitlines()))      # the docstring's table, of this run


def G(t):
    return None if t is None else t.to(DEV).contiguous()


def shift_of(F):
    """F = 1 and F = 257: the single row / the one row of the last block is a front-facing seam sample whose tr = 1.1 is clamped."""
    return PR.shift_for(F - 1, cos="front", tr="above", texel="seam", rough="mid") if F in (1, 257) else 0


@functools.lru_cache(maxsize=3)
def case(F, hw, indirect):
    """(problem, emitter): the pmf the kernels read is the one the library builds from the image; the references get the same table."""
    from intrinsicavatar_amd import pbr
    p = PR.make_problem(F, hw, seed=1, shift=shift_of(F), indirect=indirect)
    e = pbr.EnvironmentLightTensor(G(p["base"]))
    e.update_pdf()
    pmf = e.pmf.cpu()
    assert torch.equal(pmf == 0, p["pmf"] == 0) and int((pmf == 0).sum()) == len(PR.zero_texels(*hw))
    p["pmf"] = pmf
    return p, e


@functools.lru_cache(maxsize=8)
def refs(F, hw, indirect, mode, subset, env_grad=True):
    p, _ = case(F, hw, indirect)
    r64, t32 = PR.shade_ref(p, mode, F64, SUBSETS[subset], env_grad), PR.shade_ref(p, mode, F32, SUBSETS[subset], env_grad)
    for k in ("x0", "x1", "y0", "y1", "flag", "pdf_y", "pdf_x", "masked", "need_env", "lit", "front", "pdf_zero", "pdf_branch", "mis_on"):
        assert torch.equal(r64["dec"][k], t32["dec"][k]), k           # the generator's promise, for the pmf table of the device too
    return r64, t32


def compare_rows(what, pars, p, got, ref64, twin32):
    """the rule over ALL rows, one comparison per roughness class; a class whose reference is identically zero must be exactly zero."""
    got = got.detach().cpu()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    for name, m in PR.row_groups(p).items():
        if not bool(m.any()):
            continue
        if float(ref64[m].abs().max()) == 0.0:
            assert bool((got[m] == 0).all()), f"{what} {pars} rough={name}: expected exact zeros"
        else:
            compare(f"{what} {pars} rough={name}", got[m], ref64[m], twin32[m])


def assert_rows_zero(what, t, rows):
    t = t.detach().cpu()[rows]
    assert torch.equal(t, torch.zeros_like(t)), f"{what}: rows of a masked class are not exactly zero"


# ----------------------------------------------------------------------------------------------------------------------
# forward of the four estimators
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("mode", list(PR.MODES))
def test_shade_forward(mode, F):
    """ia_pbr_shade modes 0-3: Lo, Lo_diff, Lo_spec (vis in mode 1) on the 5 x 7 and 16 x 32 maps, with and without indirect radiance."""
    from intrinsicavatar_amd import pbr
    for hw in ((5, 7), (16, 32)):
        for indirect in (False, True):
            p, e = case(F, hw, indirect)
            r64, t32 = refs(F, hw, indirect, mode, "all")
            out = pbr.pbr_shade(mode, G(p["n"]), G(p["albedo"]), G(p["rough"]), G(p["metal"]), G(p["view_dirs"]), G(p["wo"]), G(p["tr"]),
                                G(p["ind"]), e, G(p["R"]), inv_pdf=G(p["inv_pdf"]))
            pars = f"F={F} map={hw[0]}x{hw[1]} ind={int(indirect)}"
            dark = r64["dec"]["masked"] | ~r64["dec"]["lit"]
            for k, got in zip(("Lo", "Lo_diff", "Lo_spec"), out):
                compare_rows(f"shade {mode} {k}", pars, p, got, r64[k], t32[k])
                assert_rows_zero(f"shade {mode} {k}", got, dark)
            back = PR.mask_of(p["lab"]["cos"], "nov_neg")
            assert_rows_zero(f"shade {mode} Lo_spec back-facing", out[2], back)
            if mode == "uniform_light":
                assert torch.equal(out[3].cpu(), t32["vis"])                 # 2 x the clamped, masked transmittance: exact in fp32
                assert_rows_zero("vis", out[3], r64["dec"]["masked"])


# ----------------------------------------------------------------------------------------------------------------------
# backward
def run_backward(p, e, mode, subset, env_grad=True):
    from intrinsicavatar_amd import pbr
    leaf = lambda t: G(t).clone().requires_grad_(True)      # noqa: E731
    n, alb, rough, metal = leaf(p["n"]), leaf(p["albedo"]), leaf(p["rough"][:, None]), leaf(p["metal"][:, None])
    base = leaf(p["base"]) if env_grad else G(p["base"])
    outs = pbr.pbr_shade_differentiable(mode, n, alb, rough, metal, G(p["view_dirs"]), G(p["wo"]), G(p["tr"]), G(p["ind"]), e, G(p["R"]),
                                        inv_pdf=G(p["inv_pdf"]) if mode == "uniform_light" else None, env_base=base)
    L = sum((G(p["ups"][k]) * o).sum() for k, o in enumerate(outs) if SUBSETS[subset][k])
    L.backward()
    return dict(g_normal=n.grad, g_albedo=alb.grad, g_roughness=rough.grad[:, 0], g_metallic=metal.grad[:, 0],
                g_env=base.grad if env_grad else None)


def check_point_grads(tag, pars, p, got, r64, t32):
    for k in POINT_GRADS:
        compare_rows(f"{tag} {k}", pars, p, got[k], r64[k], t32[k])
        assert_rows_zero(f"{tag} {k}", got[k], r64["dec"]["masked"])
    assert_rows_zero(f"{tag} g_roughness back-facing", got["g_roughness"], PR.mask_of(p["lab"]["cos"], "nov_neg"))


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("mode", ["light", "uniform_light"])
def test_shade_backward_per_point_gradients(mode, F):
    """ia_pbr_shade_bwd through pbr.pbr_shade_differentiable: g_normal, g_albedo, g_roughness, g_metallic for gradients arriving on Lo only,
    Lo_diff only, Lo_spec only (the absent ones are NULL pointers) and on all three; inv_pdf varies per sample.  The texel gradient of these
    small batches (direct atomics) is compared too.  Without a gradient for the image (g_env_base NULL) the four are bit-identical."""
    for hw, indirect in (((16, 32), True), ((5, 7), False)):
        p, e = case(F, hw, indirect)
        for subset in SUBSETS:
            r64, t32 = refs(F, hw, indirect, mode, subset)
            got = run_backward(p, e, mode, subset)
            pars = f"F={F} map={hw[0]}x{hw[1]} ind={int(indirect)} from={subset}"
            check_point_grads(f"bwd {mode}", pars, p, got, r64, t32)
            if float(r64["g_env"].abs().max()) == 0.0:
                assert bool((got["g_env"] == 0).all())
            else:
                compare(f"bwd {mode} g_env direct {pars}", got["g_env"], r64["g_env"], t32["g_env"], atomic_adds=PR.texel_adds(r64["dec"], hw))
            if subset == "all":
                no_env = run_backward(p, e, mode, subset, env_grad=False)
                for k in POINT_GRADS:
                    assert torch.equal(no_env[k], got[k]), k


def env_case(path, mode, F, hw, monkeypatch):
    """one texel-gradient path against the fp64 autograd of env_eval_t; returns the gradients and the direct path's for the same inputs."""
    p, e = case(F, hw, True)
    r64, t32 = refs(F, hw, True, mode, "all")
    for k in ("IA_ENV_GRAD_ATOMIC", "IA_ENV_GRAD_UNBINNED"):
        monkeypatch.delenv(k, raising=False)
    if path == "unbinned":
        monkeypatch.setenv("IA_ENV_GRAD_UNBINNED", "1")
    if path == "direct" and F >= BIG:
        monkeypatch.setenv("IA_ENV_GRAD_ATOMIC", "1")
    got = run_backward(p, e, mode, "all")
    pars = f"F={F} map={hw[0]}x{hw[1]}"
    adds = 0 if path == "fixed" else PR.texel_adds(r64["dec"], hw)
    compare(f"bwd {mode} g_env {path} {pars}", got["g_env"], r64["g_env"], t32["g_env"], atomic_adds=adds)
    untouched = r64["g_env"] == 0
    assert bool((got["g_env"].cpu()[untouched] == 0).all())                   # texels no live sample touches stay exactly zero
    check_point_grads(f"bwd {mode} ({path})", pars, p, got, r64, t32)
    return p, e, got


@pytest.mark.parametrize("mode,F", [("light", 257), ("uniform_light", 257), ("light", BIG - 1)])
def test_env_texel_gradient_direct_atomics(mode, F, monkeypatch):
    """batches below 2^18 scatter with 12 float atomics per live sample: allowance for P adds per texel channel."""
    env_case("direct", mode, F, (24, 512), monkeypatch)


@pytest.mark.parametrize("mode,F,hw", [("light", BIG, (24, 512)), ("uniform_light", BIG_RAGGED, (24, 512)), ("light", BIG, (256, 512))])
def test_env_texel_gradient_fixed_point_records(mode, F, hw, monkeypatch):
    """the default record path: records binned by band (24 x 512: 3 bands of 11 rows, samples at y0 = 10 and 21 whose y1 lies in the next
    band's first row, both clamped rows; 256 x 512: 24 bands), summed in 64-bit fixed point -- NO summation allowance, the same bits in a
    second call, per-point gradients bit-identical to the direct path's."""
    p, e, got = env_case("fixed", mode, F, hw, monkeypatch)
    again = run_backward(p, e, mode, "all")
    assert torch.equal(again["g_env"], got["g_env"])
    monkeypatch.setenv("IA_ENV_GRAD_ATOMIC", "1")
    direct = run_backward(p, e, mode, "all")
    for k in POINT_GRADS:
        assert torch.equal(direct[k], got[k]), k


@pytest.mark.parametrize("mode,F", [("uniform_light", BIG), ("light", BIG_RAGGED)])
def test_env_texel_gradient_unbinned_records(mode, F, monkeypatch):
    """IA_ENV_GRAD_UNBINNED=1: every band streams all records into float LDS atomics (2 bands of 17 rows on 24 x 512).  F = 2^18 + 8193:
    `per` = 16 900 records per range, two whole strides of 8 x 1024 and a guarded 4-stride tail."""
    p, e, got = env_case("unbinned", mode, F, (24, 512), monkeypatch)
    monkeypatch.delenv("IA_ENV_GRAD_UNBINNED")
    monkeypatch.setenv("IA_ENV_GRAD_ATOMIC", "1")
    direct = run_backward(p, e, mode, "all")
    for k in POINT_GRADS:
        assert torch.equal(direct[k], got[k]), k


# ----------------------------------------------------------------------------------------------------------------------
# the scatterer route: the same backward kernel with a 1 x 1 environment and unit radiance
@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("lobes", [1, 2, 3])
def test_scatterer_eval_forward_and_backward(lobes, n):
    """pbr._ScattererEval for the lobe sets 1 (diffuse), 2 (specular), 3 (both): eval and its gradients w.r.t. normal, roughness, albedo
    and metallic against fp64 autograd of brdf_eval_t; the cosine lobe alone leaves the material gradients exactly zero."""
    from intrinsicavatar_amd import pbr
    shift = PR.shift_for(0, cos="front", rough="mid") if n == 1 else 0
    p = PR.make_problem(n, (1, 1), seed=2, shift=shift)
    g = PR.seeded(40 + n)
    ups = [torch.randn(n, 1, generator=g), torch.randn(n, 3, generator=g)]
    r64, t32 = PR.scatterer_ref(p, lobes, F64, ups), PR.scatterer_ref(p, lobes, F32, ups)
    leaf = lambda t: G(t).clone().requires_grad_(True)      # noqa: E731
    nn, alpha, alb, metal = leaf(p["n"]), leaf(p["rough"][:, None]), leaf(p["albedo"]), leaf(p["metal"][:, None])
    diff, spec = pbr._ScattererEval.apply(lobes, nn, G(-p["view_dirs"]), G(p["wo"]), alpha, alb, metal)
    pars = f"n={n}"
    unlit = ~PR.mask_of(p["lab"]["cos"], "front", "nov_neg")
    compare_rows(f"scatterer lobes{lobes} diff", pars, p, diff, r64["diff"], t32["diff"])
    compare_rows(f"scatterer lobes{lobes} spec", pars, p, spec, r64["spec"], t32["spec"])
    assert_rows_zero("diff", diff, unlit); assert_rows_zero("spec", spec, unlit)
    ((diff * G(ups[0])).sum() + (spec * G(ups[1])).sum()).backward()
    got = dict(g_normal=nn.grad, g_roughness=alpha.grad, g_albedo=alb.grad, g_metallic=metal.grad)
    for k, t in got.items():
        t = t.reshape(r64[k].shape)
        compare_rows(f"scatterer lobes{lobes} {k}", pars, p, t, r64[k], t32[k])
        assert_rows_zero(k, t, unlit)
        if lobes == 1 and k != "g_normal":
            assert bool((t == 0).all()), k
