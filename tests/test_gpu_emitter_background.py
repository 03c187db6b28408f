"""GPU: model.add_emitter -- the emitter's radiance along camera rays (configs/config.yaml:58, models/intrinsic_avatar.py:1319-1333,
:1455-1490), kernel by kernel and end to end.

Kernel level, against fp64 torch on the same fp32 inputs:
  ia_envlight_background       bit-identical to emitter.eval() of the directions the kernel itself forms (ia_transform_dirs_s2w: the same
                               device function); against fp64 within a bound DERIVED from the bilinear footprint (below, `coord_error`).
  ia_envlight_background_bwd   texel gradient against fp64 autograd of the same bilinear expression; bit-identical run to run.
  ia_vi_composite_bwd_bg       exactly the fp32 product c_r * g_rgb; against fp64 one rounding of that product.

The fp32 coordinate error (`coord_error`).  EPS = 2^-24 (half an ulp of 1).  The world direction normalize(d @ R) carries at most 8 EPS per
component (three products and two sums of terms <= 1, the norm, the division: 6 roundings, taken as 8).
  u = atan2(x, -z) / 2 pi + 1/2:  an error of 8 EPS in x and z turns the angle by <= sqrt(2) 8 EPS / r, r = sqrt(x^2 + z^2) (12 EPS / r); atan2f
      is good to 4 ulp of a result <= pi (8 pi EPS); the scaling and the sum add 3 EPS:  du = (12 EPS / r + 8 pi EPS) / 2 pi + 3 EPS, at most 1
      (at a pole r = 0 and u is arbitrary -- in fp64 as well).
  v = acos(y) / pi:  |acos(y + e) - acos(y)| <= min(2 e / sqrt(1 - y^2), 2 sqrt(e)) for e = 8 EPS (the derivative away from the poles, the
      square-root behaviour at them); acosf 4 ulp of a result <= pi, scaling: dv = that / pi + 8 EPS + 2 EPS.
  fx = u W - 1/2, fy = v H - 1/2: dfx = W du + 2 EPS W, dfy = H dv + 2 EPS H (one rounding each of a number below W / H, and the fraction).
The bilinear value is continuous and piecewise linear in (fx, fy) with slopes bounded by the difference of neighbouring texels, so
  |out - out64| <= Dx dfx + Dy dfy + 6 EPS max|texel|      (Dx / Dy: the largest difference of horizontal (wrapping) / vertical neighbours;
                                                            6 EPS: the four weights, products and three sums of the interpolation)
and never more than max - min of the map plus that rounding term (an interpolated value lies between its texels)."""
import math
from unittest import mock

import numpy as np
import pytest
import torch

from tests import backward_refs as BR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from intrinsicavatar_amd import build
    build.build()
    from intrinsicavatar_amd import _lib as L
    return L.lib()


def G(t):
    return t.to(DEV).contiguous()


def seeded(seed):
    return torch.Generator().manual_seed(seed)


def rotation(seed):
    """a non-identity rotation with no axis left in place, fp32"""
    g = seeded(seed)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=F64))
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.float().contiguous()


def env_map(seed, H, W):
    return (torch.rand(H, W, 3, generator=seeded(seed)) * 30.0).contiguous()           # values in [0, 30]


def pixel_dir(v, u):
    """world direction of equirect coordinates (u, v) in [0,1]^2 (the convention of ia_envlight_eval), fp64"""
    th, ph = v * math.pi, (u - 0.5) * 2.0 * math.pi
    return torch.stack([torch.sin(th) * torch.sin(ph), torch.cos(th), -torch.sin(th) * torch.cos(ph)], -1)


def directions(n, R, H, W, seed):
    """n SMPL-space directions whose world images R^T-rotated back include: both poles, the +-pi seam in u (both sides), texel centres,
    and random directions of lengths other than 1."""
    g = seeded(seed)
    special = [torch.tensor([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]], dtype=F64),                                       # poles
               pixel_dir(torch.tensor([0.37, 0.61], dtype=F64), torch.tensor([1e-9, 1.0 - 1e-9], dtype=F64)),      # seam, either side
               pixel_dir(torch.tensor([0.5], dtype=F64), torch.tensor([0.0], dtype=F64)),                          # on the seam: atan2(0, -1)
               pixel_dir((torch.tensor([0.0, 1.0, H - 1.0], dtype=F64) + 0.5) / H, (torch.tensor([0.0, W - 1.0, 2.0], dtype=F64) + 0.5) / W)]
    w = torch.cat(special + [torch.randn(max(n, 1), 3, generator=g, dtype=F64)])
    w = w[torch.randperm(w.shape[0], generator=g)] if n >= w.shape[0] else w
    if n >= 63:                                               # the special directions are all present, in shuffled places
        w = torch.cat([torch.cat(special), torch.randn(n, 3, generator=g, dtype=F64)])[:n]
        w = w[torch.randperm(n, generator=g)]
    else:
        w = w[:n]
    scale = 0.25 + 2.0 * torch.rand(w.shape[0], 1, generator=g, dtype=F64)
    return ((w * scale) @ R.double().T).float().contiguous()        # d @ R == w * scale up to rounding (R orthonormal)


def world64(d, R):
    x = d.double() @ R.double()
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-6)


def footprint64(dw, H, W):
    u = torch.atan2(dw[:, 0], -dw[:, 2]) / (2 * math.pi) + 0.5
    v = torch.acos(dw[:, 1].clamp(-1, 1)) / math.pi
    fx, fy = u * W - 0.5, v * H - 0.5
    x0f, y0f = torch.floor(fx), torch.floor(fy)
    ax, ay = fx - x0f, fy - y0f
    x0, y0 = x0f.long(), y0f.long()
    return x0 % W, (x0 + 1) % W, y0.clamp(0, H - 1), (y0 + 1).clamp(0, H - 1), ax, ay


def bilinear64(base, dw):
    """the bilinear expression of ia_envlight_eval in the dtype of `base` (wrap in u, clamp in v); differentiable w.r.t. base"""
    H, W, _ = base.shape
    x0, x1, y0, y1, ax, ay = footprint64(dw, H, W)
    ax, ay = ax[:, None], ay[:, None]
    return (1 - ax) * (1 - ay) * base[y0, x0] + ax * (1 - ay) * base[y0, x1] + (1 - ax) * ay * base[y1, x0] + ax * ay * base[y1, x1]


def coord_error(dw, H, W):
    """(dfx, dfy) per ray: the module docstring"""
    r = torch.sqrt(dw[:, 0] ** 2 + dw[:, 2] ** 2)
    du = ((12 * EPS / r.clamp_min(1e-300) + 8 * math.pi * EPS) / (2 * math.pi) + 3 * EPS).clamp(max=1.0)
    e = 8 * EPS
    s = torch.sqrt((1 - dw[:, 1] ** 2).clamp_min(0))
    dth = torch.minimum(2 * e / s.clamp_min(1e-300), torch.full_like(s, 2 * math.sqrt(e)))
    dv = dth / math.pi + 10 * EPS
    return W * du + 2 * EPS * W, H * dv + 2 * EPS * H


def neighbour_differences(base):
    b = base.double()
    Dx = float((b - torch.roll(b, -1, 1)).abs().max())
    Dy = float((b[1:] - b[:-1]).abs().max()) if b.shape[0] > 1 else 0.0
    return Dx, Dy


def background(lib, d, R, base):
    from intrinsicavatar_amd import _lib as L
    n = d.shape[0]
    H, W, _ = base.shape
    out = torch.full((n, 3), -7.0, device=DEV)
    L.check(lib.ia_envlight_background(L.i64(n), L.ptr(G(d) if n else None), L.ptr(G(R)), L.ptr(G(base)), L.i32(H), L.i32(W),
                                       L.ptr(out if n else None), L.stream()), "ia_envlight_background")
    return out


@pytest.mark.parametrize("hw", [(4, 8), (16, 32)])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 200])
def test_envlight_background_forward(lib, n, hw):
    from intrinsicavatar_amd import pbr
    H, W = hw
    R, base = rotation(3), env_map(5, H, W)
    d = directions(n, R, H, W, seed=100 + n)
    out = background(lib, d, R, base)
    if n == 0:
        return
    assert bool(torch.isfinite(out).all())
    # (1) bit-identical to emitter.eval() of the kernel's own world directions
    env = pbr.EnvironmentLightTensor(G(base))
    dw32 = pbr.transform_dirs_s2w(G(d), G(R))
    assert torch.equal(out, env.eval(dw32))
    assert torch.equal(out, env.background(G(d), G(R)))
    # the exposed directions are the fp64 ones up to the 8 EPS per component the derivation assumes
    dw64 = world64(d, R)
    assert float((dw32.cpu().double() - dw64).abs().max()) <= 8 * EPS
    # (2) the derived bound against fp64
    ref = bilinear64(base.double(), dw64)
    dfx, dfy = coord_error(dw64, H, W)
    Dx, Dy = neighbour_differences(base)
    rnd = 6 * EPS * float(base.max())
    bar = torch.minimum(Dx * dfx + Dy * dfy, torch.full_like(dfx, float(base.max() - base.min()))) + rnd
    err = (out.cpu().double() - ref).abs().max(-1)[0]
    away = torch.sqrt(dw64[:, 0] ** 2 + dw64[:, 2] ** 2) > 1e-3                        # not at a pole
    print(f"BG n={n} {H}x{W}: max err {float(err.max()):.3e} (away from the poles {float(err[away].max()) if bool(away.any()) else 0.0:.3e})  median bar {float(bar.median()):.3e}  max err/bar {float((err / bar).max()):.3f}")
    assert bool((err <= bar).all()), (float((err / bar).max()), int((err > bar).sum()))
    if n >= 63:
        assert float(bar.median()) < 1e-3 * float(base.max()), "the bound must bite on ordinary directions"


def background_bwd(lib, d, R, g_out, H, W, into=None):
    from intrinsicavatar_amd import _lib as L
    n = d.shape[0]
    g_base = torch.zeros((H, W, 3), device=DEV) if into is None else into
    acc = torch.full((H, W, 3), 77, dtype=torch.int64, device=DEV)          # cleared by the entry point
    gmax = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    L.check(lib.ia_envlight_background_bwd(L.i64(n), L.ptr(G(d)), L.ptr(G(R)), L.ptr(G(g_out)), L.i32(H), L.i32(W), L.ptr(g_base),
                                           L.ptr(acc), L.ptr(gmax), L.stream()), "ia_envlight_background_bwd")
    return g_base


def bwd_directions(n, R, seed):
    """random directions up to 2.6 degrees from the poles (|y| <= 0.999: the coordinate error stays small, so the bound below bites);
    the rows above fy = 0 and below fy = H - 1 (the clamped y1 == y0 footprints) are well covered on both maps"""
    g = seeded(seed)
    w = torch.randn(4 * n + 64, 3, generator=g, dtype=F64)
    w = w / w.norm(dim=-1, keepdim=True)
    w = w[w[:, 1].abs() <= 0.999][:n]
    assert w.shape[0] == n
    return (w @ R.double().T).float().contiguous()


@pytest.mark.parametrize("hw", [(4, 8), (16, 32)])
@pytest.mark.parametrize("n", [65, 5000])
def test_envlight_background_bwd(lib, n, hw):
    """d L / d texels.  Bound per texel channel, derived:
      * the kernel's weights are those of ITS fp32 coordinates: a corner weight differs from the fp64 one by at most dfx + dfy (|d w / d ax|,
        |d w / d ay| <= 1), and a coordinate within that distance of a cell border may put its footprint one cell further: every texel of
        the 4 x 4 neighbourhood of the fp64 footprint is charged (dfx + dfy) |g| for the ray;
      * a contribution w g is formed in fp32 from (1 - ax), (1 - ay), their product and the product with g: 4 roundings, 4 EPS |w g|;
      * it is rounded to the fixed-point grid 1 / S, S = 2^shift / max|g|, shift = 62 - ceil(log2 n): max|g| 2^-(shift + 1) each, at most n per
        texel; the integer sum (global 64-bit integer atomics) is exact; the conversion back to fp32 rounds once: EPS |sum|.
    Two runs are bit-identical (integer sums do not depend on the order)."""
    H, W = hw
    R = rotation(11)
    d = bwd_directions(n, R, seed=7 + n)
    g = seeded(n)
    g_out = (torch.randn(n, 3, generator=g) * 2.0).contiguous()
    g_out[::7, 1] = 0.0                                                        # zero channel gradients are skipped by the kernel
    got = background_bwd(lib, d, R, g_out, H, W)
    again = background_bwd(lib, d, R, g_out, H, W)
    assert torch.equal(got, again), "the texel gradient must be bit-reproducible run to run"
    # accumulates (+=) into what is there
    pre = torch.full((H, W, 3), 0.5, device=DEV)
    acc = background_bwd(lib, d, R, g_out, H, W, into=pre.clone())
    assert torch.equal(acc, pre + got)
    dw64 = world64(d, R)
    base = torch.zeros(H, W, 3, dtype=F64, requires_grad=True)
    (bilinear64(base, dw64) * g_out.double()).sum().backward()
    ref = base.grad
    x0, x1, y0, y1, ax, ay = footprint64(dw64, H, W)
    if (H, W) == (4, 8) and n == 5000:
        assert int(torch.bincount(y0 * W + x0, minlength=H * W).max()) >= 128, "many rays land in one texel (more than a wave's worth)"
    dfx, dfy = coord_error(dw64, H, W)
    ga = g_out.double().abs()
    charge = (dfx + dfy)[:, None] * ga                                          # [n,3]
    bound = torch.zeros(H * W, 3, dtype=F64)
    y0u = torch.floor(torch.acos(dw64[:, 1].clamp(-1, 1)) / math.pi * H - 0.5).long()      # unclamped row
    for dy in (-1, 0, 1, 2):
        for dx in (-1, 0, 1, 2):
            bound.index_add_(0, (y0u + dy).clamp(0, H - 1) * W + (x0 + dx) % W, charge)
    absum = torch.zeros(H, W, 3, dtype=F64, requires_grad=True)
    (bilinear64(absum, dw64) * ga).sum().backward()                            # sum |w g| per texel
    shift = 62 - math.ceil(math.log2(n))
    fixed = n * float(ga.max()) * 2.0 ** -(shift + 1)
    bar = bound.reshape(H, W, 3) + 4 * EPS * absum.grad + fixed + EPS * ref.abs()
    err = (got.cpu().double() - ref).abs()
    print(f"BG_BWD n={n} {H}x{W}: max err {float(err.max()):.3e}  max|ref| {float(ref.abs().max()):.3e}  max err/bar {float((err / bar).max()):.3f}"
          f"  max bar/|ref|max {float(bar.max() / ref.abs().max()):.3e}")
    assert float(ref.abs().max()) > 0
    assert bool((err <= bar).all()), float((err / bar).max())
    # the bound must bite: one lost or misplaced ray moves a texel by its weight (1/4 on average) times |g|; the bar stays below a quarter of that
    assert float(bar.max()) < 0.25 * 0.25 * float(ga.mean()), (float(bar.max()), float(ga.mean()))


def test_emitter_background_autograd_is_the_backward_kernel(lib):
    """pbr.emitter_background / EnvironmentLightTensor.background / EnvironmentLightSG.background: gradient to the texels only, = the kernel"""
    from intrinsicavatar_amd import pbr
    H, W, n = 16, 32, 300
    R = rotation(2)
    d = bwd_directions(n, R, seed=1)
    base = G(env_map(9, H, W)).requires_grad_(True)
    dd = G(d).requires_grad_(True)
    g_out = torch.randn(n, 3, generator=seeded(4))
    out = pbr.emitter_background(base, dd, G(R))
    assert torch.equal(out.detach(), background(lib, d, R, base.detach().cpu()))
    out.backward(G(g_out))
    assert dd.grad is None, "directions get no gradient"
    assert torch.equal(base.grad, background_bwd(lib, d, R, g_out, H, W))
    sg = pbr.EnvironmentLightSG(num_SGs=8, base_res=8).to(DEV)
    img = sg.generate_image()
    bg = sg.background(G(d), G(R), env_base=img)
    assert torch.equal(bg.detach(), pbr.EnvironmentLightTensor(img.detach()).background(G(d), G(R)))
    bg.sum().backward()
    assert float(sg.mu.grad.abs().max()) > 0, "the lobes receive gradient through their image"
    assert torch.equal(sg.background(G(d), G(R)), bg.detach()), "default: the current image of the lobes"


def test_vi_composite_bwd_bg(lib):
    """the parameter set of backward_refs.vi_composite (empty rays, foreground-only rays, mixed rays, more than 64 foreground re-samples
    on a ray) against vi_composite_ref's own autograd with bg_rays.requires_grad: exact against the fp32 replay (c_r g is ONE fp32
    product), one rounding of that product against fp64."""
    from intrinsicavatar_amd import _lib as L
    p = BR.make_vi_composite_problem(seed=4)
    n = p["n_rays"]
    empty, some_bg = p["rpi"][:, 1] <= 0, p["bg_cnt"] > 0
    assert bool(empty.any()) and bool((~empty & some_bg).any()) and bool((~empty & ~some_bg).any()) and int(p["fg_ray_cnt"].max()) > 64
    rpi, bgc, T, g_rgb = (G(p[k]) for k in ("rpi", "bg_cnt", "T", "g_rgb"))
    got = torch.full((n, 3), 9.0, device=DEV)
    L.check(lib.ia_vi_composite_bwd_bg(L.i64(n), L.ptr(rpi), L.ptr(bgc), L.ptr(T), L.ptr(g_rgb), L.ptr(got), L.stream()), "ia_vi_composite_bwd_bg")

    def ref(dtype):
        """vi_composite_ref(p, True, dtype) with bg_rays a leaf of that dtype (`.to(dtype)` hands the same tensor on) and its gradient taken
        in the function's own autograd.grad call"""
        q = dict(p, bg_rays=p["bg_rays"].to(dtype).clone().requires_grad_(True))
        grad, box = torch.autograd.grad, {}

        def with_bg(outputs, inputs, **kw):
            res = grad(outputs, list(inputs) + [q["bg_rays"]], **kw)
            box["g"] = res[-1]
            return res[:-1]
        with mock.patch.object(torch.autograd, "grad", with_bg):
            BR.vi_composite_ref(q, True, dtype)
        return box["g"]
    r64, r32 = ref(F64), ref(F32)
    assert torch.equal(got.cpu(), r32), "one fp32 product per element: the replay is exact"
    assert bool(((got.cpu().double() - r64).abs() <= EPS * r64.abs()).all())
    c = torch.where(empty, torch.ones(n), torch.where(some_bg, p["T"], torch.zeros(n)))
    assert torch.equal(got.cpu(), c[:, None] * p["g_rgb"])
    assert bool((got.cpu()[~empty & ~some_bg] == 0).all()) and torch.equal(got.cpu()[empty], p["g_rgb"][empty])


def test_vi_composite_autograd_background_rays(lib):
    """VolumeInteraction.composite(..., background_rays=): forward through the kernel's background_rays argument, gradient through
    ia_vi_composite_bwd_bg, g_T with the per-ray colour"""
    from intrinsicavatar_amd import pbr
    p = BR.make_vi_composite_problem(seed=9)
    vi = pbr.VolumeInteraction.__new__(pbr.VolumeInteraction)
    vi.n_rays, vi.F = p["n_rays"], p["F"]
    vi.resampled_packed_info, vi.fg_ray_cnt, vi.fg_start, vi.bg_counts, vi.fg_ray = (G(p[k]) for k in ("rpi", "fg_ray_cnt", "fg_start", "bg_cnt", "fg_ray"))
    w, Lo, T, bgr = (G(p[k]).requires_grad_(True) for k in ("w", "Lo", "T", "bg_rays"))
    rgb = vi.composite(w, Lo, T, G(p["bg"]), bgr)
    rgb.backward(G(p["g_rgb"]))
    rgb64, gw64, gL64, gT64 = BR.vi_composite_ref(p, True, F64)
    rgb32, gw32, gL32, gT32 = BR.vi_composite_ref(p, True, F32)
    BR.compare("composite(bg_rays) rgb", rgb, rgb64, rgb32)
    BR.compare("composite(bg_rays) g_T", T.grad, gT64, gT32)
    BR.compare("composite(bg_rays) g_w", w.grad, gw64, gw32)
    empty, some_bg = p["rpi"][:, 1] <= 0, p["bg_cnt"] > 0
    c = torch.where(empty, torch.ones(vi.n_rays), torch.where(some_bg, p["T"], torch.zeros(vi.n_rays)))
    assert torch.equal(bgr.grad.cpu(), c[:, None] * p["g_rgb"])
    # without the argument: today's behaviour, and no sixth gradient
    plain = vi.composite(w.detach(), Lo.detach(), T.detach(), G(p["bg"]))
    assert torch.equal(plain, vi.composite(w.detach(), Lo.detach(), T.detach(), G(p["bg"]), None))


# ======================================================================================================================
# End to end: the golden scene (tests/forward_golden.gpu_scene) with add_emitter, against the reference's own forward_
# (tests/golden/golden_emitter.npz, make_golden_emitter.py) and against the identity  out(True) - out(False) = c_r (E_r - b).
E2E_RUNS = {"light_16_nogi": ("light_16_nogi", False), "uniform_light_512_gi": ("uniform_light_512_gi", False), "mis_16_gi": ("mis_16_gi", False),
            "light_16_nogi_albedo_only": ("light_16_nogi", True)}
_SCENES = {}


def Tn(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def GF(lib):
    from tests import forward_golden as FG
    return FG.load()


@pytest.fixture(scope="module")
def GE():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_emitter.npz"))


def scene(GF, tag):
    from tests import forward_golden as FG
    if tag not in _SCENES:
        _SCENES.clear()                                     # one scene resident at a time (two 50 MB tables each)
        _SCENES[tag] = FG.gpu_scene(GF, tag)
    return _SCENES[tag]


def run_kwargs(GF, src):
    from tests import forward_golden as FG
    mode, spp, gi = FG.RUNS[src]
    rnd = FG.explicit_randoms(GF, src)
    light_u = rnd["stratified_u"] if mode == "uniform_light" else rnd["light_u"]
    scatter_u = None
    if "scatter_u" in rnd:
        g = seeded(0)
        scatter_u = torch.cat([torch.from_numpy(rnd["scatter_u"]), torch.rand((4096, 6), generator=g)]).to(DEV)
    args = (spp, Tn(light_u), Tn(rnd["shuffle_u"]) if "shuffle_u" in rnd else None)
    return args, dict(background_color=Tn(GF["background_color"]), global_illumination=gi, render_mode=mode, scatter_u=scatter_u)


def emitter_radiance64(rs, rays, env):
    """(E64 [n,3], bar_E [n]): the fp64 bilinear expression along the SMPL-space ray directions relight() uses, and the derived bound of
    ia_envlight_background against it (module docstring)."""
    d = rs.deformer.transform_rays_w2s(rays.float())[:, 3:6].contiguous().cpu()
    R = rs.deformer.w2s[:3, :3].contiguous().cpu()
    base = env.base.detach().cpu()
    H, W, _ = base.shape
    dw64 = world64(d, R)
    dfx, dfy = coord_error(dw64, H, W)
    Dx, Dy = neighbour_differences(base)
    return bilinear64(base.double(), dw64), Dx * dfx + Dy * dfy + 6 * EPS * float(base.max()), d, R


@pytest.mark.parametrize("tag", list(E2E_RUNS))
def test_add_emitter_end_to_end(GF, GE, tag):
    """(a) add_emitter=False is bit-identical to the call without the argument.
    (b) with identical random tensors D_gpu = out(True) - out(False) equals c_r (E_r - b): c_r from the returned resampled_packed_info,
        background counts and opacity; E_r the fp64 expression.  Bound, derived: both images are a + c x with the SAME a and c (same
        samples, same foreground radiance), each formed with at most two roundings (product, sum -- or one fma): 2 EPS (|out_T| + |out_F|);
        the kernel's E against fp64: c_r bar_E (the footprint bound of the kernel test); the product c_r (E - b) of the expectation: EPS.
    (c) against the reference: D_ref = golden_emitter - golden_forward;  |D_gpu - D_ref| <= bar_opacity |E_r - b| + the rounding term of
        (b) for both sides.  bar_opacity: this project's own bar for the opacity of these runs against the same fixture (the hard cap over
        all 784 rays, tests/test_gpu_forward_golden.BARS_EVAL["opacity"][0]; tests/golden/parity_bars.json holds the bars of other scenes
        only) -- c_r = 1 - opacity on a partly transparent ray, so an opacity that differs by that much moves D by that much of E - b.
        Rays in another discrete state than the reference's (empty / background count > 0 / background count = 0) would be left out and
        are counted: at most 0."""
    from tests.test_gpu_forward_golden import BARS_EVAL, BARS_MC
    from intrinsicavatar_amd import pbr
    src, albedo_only = E2E_RUNS[tag]
    rs, mat, env, rays = scene(GF, src)
    (spp, light_u, shuffle_u), kw = run_kwargs(GF, src)
    kw = dict(kw, albedo_only=albedo_only)
    # (a)
    plain = rs.forward_(rays, mat, env, spp, light_u, shuffle_u, **kw)
    off = rs.forward_(rays, mat, env, spp, light_u, shuffle_u, add_emitter=False, **kw)
    on = rs.forward_(rays, mat, env, spp, light_u, shuffle_u, add_emitter=True, **kw)
    assert sorted(plain) == sorted(off) == sorted(on)
    for k in plain:
        assert torch.equal(plain[k], off[k]), k
        assert on[k].shape == plain[k].shape and on[k].dtype == plain[k].dtype, k
        if not k.startswith(("comp_rgb_phys", "comp_demod_phys")):
            assert torch.equal(plain[k], on[k]), k            # `visibility` included: composited without background
    # (b)
    rF = rs.relight(rays, mat, env, spp, light_u, shuffle_u, **kw)
    rT = rs.relight(rays, mat, env, spp, light_u, shuffle_u, add_emitter=True, **kw)
    n = rays.shape[0]
    b = GF["background_color"].astype(np.float64)
    E, bar_E, d_smpl, R = emitter_radiance64(rs, rays, env)
    E, bar_E = E.numpy(), bar_E.numpy()
    opac = rT["opacity"].cpu().numpy()[:, 0]
    if "resampled_packed_info" in rT and not albedo_only:
        cnt = rT["resampled_packed_info"].cpu().numpy()[:, 1]
        bgc = rT["bg_counts"].cpu().numpy()
        state = np.where(cnt <= 0, 0, np.where(bgc > 0, 1, 2))                    # 0 empty, 1 background count > 0, 2 background count = 0
    else:
        state = np.zeros(n, np.int64)                                             # albedo_only / no samples: the emitter on every ray
    T32 = (1.0 - rT["opacity"]).cpu().numpy()[:, 0].astype(np.float64)           # the transmittance relight() hands to the kernel
    c = np.where(state == 0, 1.0, np.where(state == 1, T32, 0.0))
    assert torch.equal(rT["opacity"], rF["opacity"])
    print(f"E2E {tag}: rays empty {int((state == 0).sum())}, background count > 0 {int((state == 1).sum())}, = 0 {int((state == 2).sum())};"
          f" max E {E.max():.2f}")
    if not albedo_only:
        assert all(int((state == s).sum()) > 0 for s in (0, 1, 2)), "all three values of c_r occur"
    for key in ("comp_rgb_phys", "comp_demod_phys"):
        oT, oF = rT[key].cpu().numpy().astype(np.float64), rF[key].cpu().numpy().astype(np.float64)
        want = c[:, None] * (E - b[None])
        rnd = 2 * EPS * (np.abs(oT) + np.abs(oF)) + (c * bar_E)[:, None] + EPS * np.abs(want)
        D_gpu = oT - oF
        err = np.abs(D_gpu - want)
        print(f"E2E {tag} {key}: identity max err {err.max():.3e}  max err/bound {(err / rnd).max():.3f}  max |D| {np.abs(D_gpu).max():.3f}")
        assert (err <= rnd).all(), (key, float((err / rnd).max()))
        assert np.array_equal(D_gpu[state == 2], np.zeros_like(D_gpu[state == 2]))
        # empty rays carry the emitter's radiance exactly
        bg32 = env.background(Tn(d_smpl.numpy()), Tn(R.numpy())).detach().cpu().numpy()
        assert np.array_equal(rT[key].cpu().numpy()[state == 0], bg32[state == 0])
        # (c)
        ref_T, ref_F = GE[f"{tag}_{key}"].astype(np.float64), GF[f"{src}_out_{key}"].astype(np.float64)
        if albedo_only:                                                           # the reference without the emitter: the colour on every ray
            ref_F = np.broadcast_to(b[None], ref_T.shape)
        D_ref = ref_T - ref_F
        ref_opac = GF[f"{src}_out_opacity"][:, 0]
        if albedo_only:
            ref_state = np.zeros(n, np.int64)
        else:
            moved = np.abs(E - b[None]).max(-1) > 1e-3
            ref_zero = (np.abs(D_ref).max(-1) == 0) & moved
            ref_state = np.where(ref_zero, 2, np.where(ref_opac == 0, 0, 1))
            gpu_cmp = np.where(state == 2, 2, np.where(opac == 0, 0, 1))          # an empty ray and one of opacity 0 carry the same c_r = 1
            state_cmp = gpu_cmp
        left_out = (ref_state != (np.zeros(n, np.int64) if albedo_only else state_cmp))
        print(f"E2E {tag} {key}: rays in another discrete state than the reference's: {int(left_out.sum())}")
        assert int(left_out.sum()) <= 0
        bar_op = BARS_EVAL["opacity"][0]
        rnd_ref = 2 * EPS * (np.abs(ref_T) + np.abs(ref_F)) + (c * bar_E)[:, None]
        bound = bar_op * np.abs(E - b[None]) + rnd + rnd_ref
        err = np.abs(D_gpu - D_ref)[~left_out]
        print(f"E2E {tag} {key}: |D_gpu - D_ref| max {err.max():.3e}  max err/bound {(err / bound[~left_out]).max():.3f}")
        assert (err <= bound[~left_out]).all(), (key, float((err / bound[~left_out]).max()))
        # the sRGB forms: the Monte-Carlo part is the add_emitter=False image's (this project's bar for it against the same fixture),
        # the emitter part moves by at most the bound above times the largest slope of the sRGB curve (12.92)
        full_gpu, full_ref = on[key + "_full"].cpu().numpy().astype(np.float64), GE[f"{tag}_{key}_full"].astype(np.float64)
        assert np.array_equal(on[key + "_full"].cpu().numpy(), pbr.rgb_to_srgb(rT[key]).clamp(0, 1).cpu().numpy())
        mc = 0.0 if albedo_only else BARS_MC[src][key + "_full"][0]
        errf = np.abs(full_gpu - full_ref)
        assert (errf <= mc + 12.92 * bound + 4 * EPS).all(), (key, float(errf.max()))
        assert np.array_equal(on[key].cpu().numpy(), rT[key].cpu().numpy())


def test_model_forward_passes_add_emitter_chunk_by_chunk(GF):
    from intrinsicavatar_amd import system
    rs, mat, env, rays = scene(GF, "light_16_nogi")
    (spp, light_u, shuffle_u), kw = run_kwargs(GF, "light_16_nogi")
    whole = rs.forward_(rays, mat, env, spp, light_u, shuffle_u, add_emitter=True, **kw)
    chunked = system.model_forward(rs, rays, mat, env, spp, light_u, shuffle_u, ray_chunk=300, move_to_cpu=False, add_emitter=True, **kw)
    for k in ("comp_rgb_phys", "comp_demod_phys", "comp_rgb_phys_full"):
        assert torch.equal(whole[k], chunked[k]), k


def test_training_emitter_gradient(GF):
    """forward_train_(add_emitter=True) + reference_training_loss(rgb_wo_mask=...) on the light_16_gi_train scene: env_base.grad is
    non-zero; on the rays that are empty in this frame it equals the direct expression -- the L1 / MSE derivative of the sRGB image
    scattered through the bilinear weights, in fp64 --; with add_emitter=False those rays give the texels nothing.
    Bound of the identity, derived: the per-ray gradient passes the fp32 sRGB curve and the two means (a pow, a few products: 16 EPS
    relative) at a radiance that is the fp64 one up to the forward bound bar_E, then the scatter of the backward kernel test (coordinate-error charge on the 4 x 4 neighbourhood, 4 EPS of sum |w g|, one
    rounding of the sum).  A channel within 1e-5 of a kink of the curve (0, 0.0031308, 1) may sit on the other branch: charged in full."""
    from tests import forward_golden as FG
    from intrinsicavatar_amd import train_phys
    tag = FG.TRAIN_RUN
    rs, mat, env, rays = scene(GF, tag)
    rnd = FG.explicit_randoms(GF, tag)
    g = seeded(0)
    mj = torch.cat([torch.from_numpy(rnd["material_jitter"]), torch.randn((4096, 3), generator=g)]).to(DEV)
    lu = torch.cat([torch.from_numpy(rnd["light_u"]), torch.rand((4096, 3), generator=g)]).to(DEV)
    n = rays.shape[0]
    target = torch.rand((n, 3), generator=g).to(DEV)
    alpha = (torch.rand(n, generator=g) > 0.5).float().to(DEV)
    lam = dict(lambda_rgb_phys_l1=1.0, lambda_rgb_phys_mse=0.5)
    kw = dict(jitter=Tn(rnd["near_jitter"]), material_jitter=mj, background_color=Tn(GF["background_color"]), global_illumination=True,
              render_mode="light")

    def run(add_emitter):
        base = env.base.detach().clone().requires_grad_(True)
        d = rs.forward_train_(rays, mat, env, 16, lu, env_base=base, add_emitter=add_emitter, **kw)
        loss, terms = train_phys.reference_training_loss(d, target, alpha, lam, mat, rgb_wo_mask=target if add_emitter else None)
        return d, base, loss, terms

    def share(d, sel):
        """the share of the two physically based terms (means over ALL n rays and 3 channels) that the rays `sel` hold"""
        diff = d["comp_rgb_phys_full"][sel] - target[sel]
        return (lam["lambda_rgb_phys_l1"] * diff.abs().sum() + lam["lambda_rgb_phys_mse"] * (diff ** 2).sum()) / (3 * n)
    d, base_leaf, loss, terms = run(True)
    g_full, = torch.autograd.grad(loss, base_leaf, retain_graph=True)
    assert float(g_full.abs().max()) > 0
    # all rays enter the physically based terms
    full = d["comp_rgb_phys_full"].detach()
    assert torch.allclose(terms["rgb_phys_l1"].detach(), (full - target).abs().mean()) and \
        torch.allclose(terms["rgb_phys_mse"].detach(), ((full - target) ** 2).mean())
    assert torch.allclose(share(d, torch.arange(n, device=DEV)).detach(),
                          (lam["lambda_rgb_phys_l1"] * terms["rgb_phys_l1"] + lam["lambda_rgb_phys_mse"] * terms["rgb_phys_mse"]).detach())
    has = torch.zeros(n, dtype=torch.bool, device=DEV)
    has[d["ray_indices"].long()] = True
    empty = torch.nonzero(~has)[:, 0]                       # no primary sample: no re-sample either
    assert 100 < empty.numel() < n
    g_e, = torch.autograd.grad(share(d, empty), base_leaf)
    d_off, base_off, _, _ = run(False)
    s_off = share(d_off, empty)
    if s_off.requires_grad:
        g_off, = torch.autograd.grad(s_off, base_off, allow_unused=True)
        assert g_off is None or float(g_off.abs().max()) == 0.0
    assert torch.equal(d_off["comp_rgb_phys"][empty], Tn(GF["background_color"])[None].expand(empty.numel(), 3))
    r_e = rays[empty].contiguous()
    # the direct expression, fp64
    E, bar_E, d_smpl, R = emitter_radiance64(rs, r_e, env)
    base = env.base.detach().cpu()
    H, W, _ = base.shape
    dw64 = world64(d_smpl, R)
    t = target[empty].cpu().double()
    m = empty.numel()
    x = E.clamp(0, 1)
    srgb = torch.where(x <= 0.0031308, x * 12.92, x.clamp_min(0.0031308) ** (1 / 2.4) * 1.055 - 0.055)
    dsrgb = torch.where(x <= 0.0031308, torch.full_like(x, 12.92), 1.055 / 2.4 * x.clamp_min(0.0031308) ** (1 / 2.4 - 1))
    dsrgb = torch.where((E > 0) & (E < 1), dsrgb, torch.zeros_like(dsrgb))
    g_ray = (lam["lambda_rgb_phys_l1"] * torch.sign(srgb - t) + lam["lambda_rgb_phys_mse"] * 2 * (srgb - t)) / (3 * n) * dsrgb
    leaf = torch.zeros(H, W, 3, dtype=F64, requires_grad=True)
    (bilinear64(leaf, dw64) * g_ray).sum().backward()
    ref = leaf.grad
    near_kink = ((E.abs() < 1e-5) | ((E - 0.0031308).abs() < 1e-5) | ((E - 1).abs() < 1e-5) | ((srgb - t).abs() < 1e-6))
    g_max = (lam["lambda_rgb_phys_l1"] + 2 * lam["lambda_rgb_phys_mse"]) / (3 * n) * 12.92
    dfx, dfy = coord_error(dw64, H, W)
    # the kernel's radiance differs from the fp64 one by at most bar_E (the forward bound), which moves the per-ray gradient by |d g / d E| bar_E
    d2srgb = torch.where(x <= 0.0031308, torch.zeros_like(x), 1.055 / 2.4 * (1 / 2.4 - 1) * x.clamp_min(0.0031308) ** (1 / 2.4 - 2))
    dg_dE = (lam["lambda_rgb_phys_l1"] * d2srgb.abs() + lam["lambda_rgb_phys_mse"] * 2 * (dsrgb ** 2 + (srgb - t).abs() * d2srgb.abs())) / (3 * n)
    charge = (dfx + dfy)[:, None] * g_ray.abs() + near_kink.double() * g_max + bar_E[:, None] * dg_dE
    x0 = footprint64(dw64, H, W)[0]
    y0u = torch.floor(torch.acos(dw64[:, 1].clamp(-1, 1)) / math.pi * H - 0.5).long()
    bound = torch.zeros(H * W, 3, dtype=F64)
    for dy in (-1, 0, 1, 2):
        for dx in (-1, 0, 1, 2):
            bound.index_add_(0, (y0u + dy).clamp(0, H - 1) * W + (x0 + dx) % W, charge)
    absum = torch.zeros(H, W, 3, dtype=F64, requires_grad=True)
    (bilinear64(absum, dw64) * g_ray.abs()).sum().backward()
    bar = bound.reshape(H, W, 3) + 20 * EPS * absum.grad + EPS * ref.abs() + 1e-30
    err = (g_e.cpu().double() - ref).abs()
    print(f"TRAIN empty rays {m}: max |grad| {float(ref.abs().max()):.3e}  max err {float(err.max()):.3e}  max err/bar {float((err / bar).max()):.3f}"
          f"  channels near a kink {int(near_kink.sum())}")
    assert float(ref.abs().max()) > 0
    assert bool((err <= bar).all()), float((err / bar).max())
    assert float(bar.max()) < 0.05 * float(ref.abs().max()), "the bound must bite"


# ======================================================================================================================
# data.AnimationFrames and animation.render_sequence
def _write_case(GA, tag, root):
    import os
    np.savez(os.path.join(root, "cameras.npz"), **{k: GA[f"{tag}_in_cam_{k}"] for k in ("intrinsic", "extrinsic", "height", "width")})
    np.savez(os.path.join(root, "poses.npz"), poses=GA[f"{tag}_in_poses"], trans=GA[f"{tag}_in_trans"])
    ds, start, end, skip, near, far = GA[f"{tag}_cfg"]
    return dict(start=int(start), end=int(end), skip=int(skip), downscale=int(ds), near=None if np.isnan(near) else float(near),
                far=None if np.isnan(far) else float(far))


@pytest.mark.parametrize("tag", ["aist", "perframe"])
def test_animation_frames_against_the_references_dataset(lib, tag, tmp_path):
    """AnimationFrames.frame(idx) against golden_animation.npz: integers, betas, poses, transl, near, far, w2c and rays_o exact; rays_d
    within 5e-7 absolute -- the reference rotates the fp32 unit camera direction by the fp32 c2w in fp32 (1 ulp of the unit input through
    an orthonormal 3 x 3 product plus its three roundings: 4 x 2^-24 x sqrt(3) < 5e-7), ia_make_rays forms the same direction in fp64 and
    rounds once."""
    import os
    from intrinsicavatar_amd import data, io_formats
    GA = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_animation.npz"))
    kw = _write_case(GA, tag, str(tmp_path))
    hdr = np.random.default_rng(0).random((8, 16, 3)).astype(np.float32) * 4
    io_formats.save_hdr(str(tmp_path / "light.hdr"), hdr)
    fr = data.AnimationFrames.from_dir(str(tmp_path), GA["betas"], hdri_filepath=str(tmp_path / "light.hdr"), device=DEV, **kw)
    assert len(fr) == int(GA[f"{tag}_len"]) and fr.img_wh == tuple(int(v) for v in GA[f"{tag}_img_wh"])
    shared = None
    for idx in range(len(fr)):
        b = fr.frame(idx)
        assert sorted(b) == sorted(["rays_o", "rays_d", "betas", "global_orient", "body_pose", "transl", "index", "w2c", "near", "far", "hdri"])
        for k in ("betas", "global_orient", "body_pose", "transl", "index", "w2c", "near", "far", "rays_o"):
            ref = GA[f"{tag}_{idx}_{k}"]
            got = b[k].cpu().numpy()
            assert got.shape == (1,) + ref.shape and got.dtype == ref.dtype, (k, got.shape, ref.shape, got.dtype, ref.dtype)
            assert np.array_equal(got[0], ref), (k, idx)
        err = np.abs(b["rays_d"].cpu().numpy()[0].astype(np.float64) - GA[f"{tag}_{idx}_rays_d"].astype(np.float64)).max()
        print(f"ANIM {tag} frame {idx}: rays_d max err {err:.3e}")
        assert err <= 5e-7
        assert tuple(b["hdri"].shape) == (1, 1024, 2048, 3)
        shared = b["hdri"] if shared is None else shared
        assert b["hdri"].data_ptr() == shared.data_ptr(), "one HDRI, loaded once and shared by the frames"
    with pytest.raises(IndexError):
        fr.frame(len(fr))


def test_render_sequence(lib, tmp_path):
    """three frames of 16 x 16 rays of the synthetic model at spp 16: resample_light=False reuses ONE light_u and its frame 0 equals a direct
    forward_ call with that light_u bit for bit; resample_light=True draws per frame; with add_emitter=True empty rays equal
    emitter.background exactly."""
    import os
    from intrinsicavatar_amd import animation, data, fields, smpl, system, synthetic as S
    GA = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_animation.npz"))
    np.savez(str(tmp_path / "cameras.npz"), intrinsic=np.eye(3), extrinsic=np.eye(4), height=np.int64(1080), width=np.int64(1080))
    np.savez(str(tmp_path / "poses.npz"), poses=GA["aist_in_poses"], trans=GA["aist_in_trans"])
    host = data.animation_host(str(tmp_path), np.zeros(10), start=0, end=8, skip=4, downscale=67.5)
    assert (host["height"], host["width"]) == (16, 16)
    hdri = (np.random.default_rng(1).random((8, 16, 3)) * 30).astype(np.float32)
    frames = data.AnimationFrames(host, hdri, DEV)
    rs, _, _ = S.build_frame(DEV, 16, 16, pose_seed=0, beta=0.01, num_samples_per_ray=64, grid_D=16, grid_H=64, grid_W=64, smooth_iters=5,
                             hash_amp=2e-3)
    mat = fields.VolumeMaterial(seed=2).to(DEV)
    eye = torch.eye(24, device=DEV)
    body = smpl.SMPLKinematics(torch.from_numpy(S.JOINTS).to(DEV), torch.zeros((24, 3, 10), device=DEV), torch.zeros((207, 72), device=DEV),
                               eye, S.PARENTS.tolist(), eye)
    kw = dict(cano_pose=(0.0, 0.0, 0.0, 0.0), occ_res=32)
    lights = {}
    for resample in (False, True):
        gen = torch.Generator().manual_seed(5)
        seen = []
        for idx, out in animation.render_sequence(rs, mat, frames, body, 16, add_emitter=True, resample_light=resample, generator=gen,
                                                       ray_chunk=100 if resample else 1 << 19, **kw):      # chunked: one num_samples entry per chunk
            seen.append(out["light_u"].clone())
            assert tuple(out["comp_rgb_phys"].shape) == (256, 3) and bool(torch.isfinite(out["comp_rgb_phys"]).all())
            batch, bg, _ = system.preprocess_data(dict(frames.frame(idx)), "test")
            rays = batch["rays"]
            emitter_bg = None
            if idx == 0 or resample:
                from intrinsicavatar_amd import pbr
                env = pbr.EnvironmentLightTensor(frames.hdri[0].contiguous())
                env.update_pdf()
                if idx == 0 and not resample:
                    direct = rs.forward_(rays, mat, env, 16, out["light_u"], out["shuffle_u"], background_color=bg, global_illumination=True,
                                         render_mode="light", add_emitter=True)
                    for k, v in direct.items():
                        assert torch.equal(v, out[k]), k
                d_smpl = rs.deformer.transform_rays_w2s(rays.float())[:, 3:6].contiguous()
                emitter_bg = env.background(d_smpl, rs.deformer.w2s[:3, :3].contiguous())
                empty = out["opacity"][:, 0] == 0
                assert int(empty.sum()) > 0
                assert torch.equal(out["comp_rgb_phys"][empty], emitter_bg[empty])
                assert torch.equal(out["comp_demod_phys"][empty], emitter_bg[empty])
            if idx == 0:
                paths = animation.save_frame(out, 16, 16, str(tmp_path / f"frame_{int(resample)}"))
                assert all(os.path.getsize(p) > 0 for p in paths.values()) and "pbr_rgb" in paths
        assert len(seen) == 3
        lights[resample] = seen
    assert torch.equal(lights[False][0], lights[False][1]) and torch.equal(lights[False][0], lights[False][2])
    assert not torch.equal(lights[True][0], lights[True][1]) and not torch.equal(lights[True][1], lights[True][2])
