"""Plain torch references of the PBR shading kernels (csrc/pbr.hip) and an input generator that BUILDS its samples per edge class.

Nothing here touches the GPU or imports the library.  The scheme is that of tests/backward_refs.py: every reference is ONE formula
that runs in the dtype of its inputs -- fed the fp32 inputs cast up it is `ref64`, fed them as they are (on the CPU) it is `twin32` --
and everything is compared with `backward_refs.compare`, so no tolerance is written down here.

For that rule to hold over ALL samples, every discrete decision of a sample (bilinear texel footprint, nearest pdf texel, cosine mask,
front / back facing, transmittance clamp, zero pmf, the pdf branch of mis / mats) must come out the same in fp32, in fp64 and on the
device.  So the generator does not draw directions and hope; it constructs them:

  * light directions from texel coordinates: floor(fx), floor(fy) are picked per texel class and the bilinear fractions ax, ay from
    [0.1, 0.4) u [0.6, 0.9); dir_to_uv is inverted in fp64 and wo = d_world @ R^T.  The gap around 0.5 keeps the nearest-texel pdf
    lookup of mode 0 (boundary at fraction 0.5) as far from its boundary as the bilinear footprint is from its own;
  * normals and view directions from prescribed cosines: |NoL| >= 0.02, |NoV| >= 0.02, |NoL + NoV| >= 0.02 (NoH of the pdf branch of
    mis / mats), |wi + wo| >= 0.1 for every row (VoH = |wi + wo| / 2: the azimuth of wi about n stays within 2.4 rad of wo's and
    |NoL| <= 0.98), plus a class with NoL EXACTLY 0 (n = e_z, wo = e_x)
    that the `> 1e-6` mask must reject.  The one fixed direction e_x @ R of that class is kept >= 0.01 texel away from every boundary of
    every map by the choice of R (`rotation()`); its radiance is multiplied by an exact 0 in every mode.

Attributes are assigned cyclically with pairwise coprime periods <= 8 on the row index i (cosine class 8, transmittance 7, texel class 5,
roughness 3) and on j = i // 8 (metallic 7, albedo 5), so every value of every attribute holds >= 32 rows of any batch of F >= 257 and
occurs among any 255 consecutive rows -- the last F % 256 rows of a large batch included.  `shift` rotates the assignment, so that a
chosen combination sits in a chosen row (the single row of F = 1, the one-row last block of F = 257): `shift_for`.
"""
import math

import torch

from tests import torch_ref as TR
from tests.backward_refs import seeded

MAPS = ((1, 1), (5, 7), (16, 32), (24, 512), (256, 512))         # (H, W)
MODES = {"light": 0, "uniform_light": 1, "mis": 2, "mats": 3}

# cyclic attribute tables ------------------------------------------------------------------------------------------------------
COS = ("front", "front", "front", "nol_neg", "front", "nol_zero", "front", "nov_neg")        # i % 8
TRS = ("interior", "zero", "one", "below", "above", "interior", "one")                      # i % 7
TR_VALUE = {"zero": 0.0, "one": 1.0, "below": -0.1, "above": 1.1}
TEXEL = ("interior", "seam", "top", "bottom", "zero_pmf")                                    # i % 5
ROUGH = ("mid", "lo", "one")                                                                 # i % 3
ROUGH_VALUE = {"lo": 0.05, "one": 1.0}
METAL = ("mid", "zero", "one", "mid", "zero", "one", "mid")                                  # (i // 8) % 7
ALBEDO = ("mid", "c0_zero", "c0_one", "mid", "c2_zero_c1_one")                               # (i // 8) % 5
MIN_ROWS = 32


def zero_texels(H, W):
    """texels of the map set to exactly 0 (pmf 0): none on maps too small to keep them off the seam and the clamped rows."""
    if H < 3 or W < 3:
        return ()
    return tuple(sorted({(H // 2, W // 2), (1, W - 2), (H - 2, 1)}))


class Labels:
    """the class name of every row for one attribute: a table of names and the per-row index into it."""

    def __init__(self, table, idx):
        self.table, self.idx = tuple(table), idx

    def __getitem__(self, row):
        return self.table[int(self.idx[row])]

    def mask(self, *values):
        return torch.tensor([t in values for t in self.table])[self.idx]

    def count(self, name):
        return int(self.mask(name).sum())

    def values(self, start=0):
        return {self.table[int(a)] for a in torch.unique(self.idx[start:])}


def labels(F, shift=0):
    """per-row class names of a batch of F rows: dict of Labels."""
    i = torch.arange(F) + int(shift)
    j = i // 8
    return dict(cos=Labels(COS, i % 8), tr=Labels(TRS, i % 7), texel=Labels(TEXEL, i % 5), rough=Labels(ROUGH, i % 3),
                metal=Labels(METAL, j % 7), albedo=Labels(ALBEDO, j % 5))


def shift_for(row, **want):
    """smallest shift that gives row `row` the wanted classes, e.g. shift_for(256, cos="front", tr="one", texel="seam")."""
    for s in range(8 * 8 * 7 * 5 * 3 * 7 * 5):
        i = row + s
        have = dict(cos=COS[i % 8], tr=TRS[i % 7], texel=TEXEL[i % 5], rough=ROUGH[i % 3], metal=METAL[(i // 8) % 7], albedo=ALBEDO[(i // 8) % 5])
        if all(have[k] == v for k, v in want.items()):
            return s
    raise ValueError(want)


def mask_of(lab, *values):
    return lab.mask(*values)


# ---- the formulas (dtype-generic) --------------------------------------------------------------------------------------------
def dir_to_uv(d):
    u = torch.atan2(d[:, 0], -d[:, 2]) / (2 * math.pi) + 0.5
    v = torch.acos(d[:, 1].clamp(-1, 1)) / math.pi
    return u, v


def uv_to_dir(u, v):
    phi, th = (u - 0.5) * 2 * math.pi, v * math.pi
    return torch.stack([torch.sin(th) * torch.sin(phi), torch.cos(th), -torch.sin(th) * torch.cos(phi)], -1)


def footprint(d, H, W):
    """what env_footprint computes: wrapped / clamped corner indices, the fractions and the y1 == y0 flag of the record."""
    u, v = dir_to_uv(d)
    fx, fy = u * W - 0.5, v * H - 0.5
    x0f, y0f = torch.floor(fx), torch.floor(fy)
    ax, ay = fx - x0f, fy - y0f
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = (x0 + 1) % W, (y0 + 1).clamp(0, H - 1)
    x0, y0 = x0 % W, y0.clamp(0, H - 1)
    return dict(x0=x0, x1=x1, y0=y0, y1=y1, ax=ax, ay=ay, flag=y1 == y0)


def pdf_texel(d, H, W):
    u, v = dir_to_uv(d)
    return (v * H).long().clamp(0, H - 1), (u * W).long().clamp(0, W - 1)


def boundary_distance(d, H, W):
    """distance (in texels) of each direction to the nearest decision boundary: of the bilinear footprint (fraction 0 / 1) and of the
    nearest-texel pdf lookup (fraction 0.5)."""
    f = footprint(d, H, W)
    dist = lambda a: torch.minimum(torch.minimum(a, 1 - a), (a - 0.5).abs())      # noqa: E731
    return torch.minimum(dist(f["ax"]), dist(f["ay"]))


def env_pmf(base):
    """sampling pmf of an equirect image: luminance x sin(theta), normalised in double (EnvironmentLightTensor.update_pdf)."""
    H = base.shape[0]
    sin_t = torch.sin((torch.arange(H, dtype=torch.float64) + 0.5) * math.pi / H)[:, None]
    lum = (0.2126 * base[..., 0] + 0.7152 * base[..., 1] + 0.0722 * base[..., 2]).clamp_min(0).double()
    w = lum * sin_t
    return (w / w.sum()).float().contiguous()


def env_pdf_t(pmf, d):
    """emitter.pdf: pmf of the nearest texel x H W / (2 pi^2 sin theta), sin of the ROW CENTRE."""
    H, W = pmf.shape
    y, x = pdf_texel(d, H, W)
    sin_t = torch.sin((y.to(d.dtype) + 0.5) * math.pi / H)
    return pmf[y, x] * (H * W / (2 * math.pi * math.pi)) / sin_t.clamp_min(1e-8)


def brdf_pdf_t(n, wi, wo, alpha):
    """MultiLobe sampling density: 1/2 cosine lobe + 1/2 GGX half-vector sampling, the latter only where NoH > 0 and VoH > 0."""
    NoL = (n * wo).sum(-1)
    h = wi + wo
    hl = h.norm(dim=-1, keepdim=True)
    h = h / hl.clamp_min(1e-30)
    NoH, VoH = (n * h).sum(-1), (wi * h).sum(-1)
    a2 = alpha ** 2
    dd = NoH ** 2 * (a2 - 1) + 1
    on = (hl[:, 0] >= 1e-12) & (NoH > 0) & (VoH > 0)
    ggx = torch.where(on, 0.5 * (a2 / (math.pi * dd ** 2)) * NoH / (4 * torch.where(on, VoH, torch.ones_like(VoH))), torch.zeros_like(NoH))
    return torch.where(NoL > 0, 0.5 * NoL / math.pi + ggx, torch.zeros_like(NoL)), on & (NoL > 0)


def scatterer_eval_t(lobes, n, wi, wo, alpha, albedo, metallic):
    """scatterer.eval of the lobe set: 1 = diffuse only, 2 = specular only, 3 = both.  (diff [P,1], spec [P,3]) incl. the cosine."""
    diff, spec = TR.brdf_eval_t(n, wi, wo, alpha, albedo, metallic)
    if lobes == 1:
        spec = torch.zeros_like(spec)
    if lobes == 2:
        diff = torch.zeros_like(diff)
    return diff[:, None], spec


def shade_t(mode, n, albedo, rough, metal, view_dirs, wo, tr, ind, inv_pdf, base, pmf, R):
    """pbr_light_kernel<mode>: (Lo, Lo_diff, Lo_spec, vis, decisions).  Directions, transmittance, indirect radiance, weights and the pmf
    are constants; differentiable in normal, albedo, roughness, metallic and the image."""
    wi = -view_dirs
    cosv = (n * wo).sum(-1)
    masked = ~(cosv > 1e-6) if mode <= 1 else torch.zeros_like(cosv, dtype=torch.bool)
    t = tr.clamp(0, 1) if mode <= 1 else tr
    t = torch.where(masked, torch.zeros_like(t), t)
    diff, spec = TR.brdf_eval_t(n, wi, wo, rough, albedo, metal)
    need_env = ~masked & ((t > 0) if mode <= 1 else torch.ones_like(masked))
    dw = wo @ R
    dw = dw / dw.norm(dim=-1, keepdim=True).clamp_min(1e-6)
    em = torch.where(need_env[:, None], TR.env_eval_t(base, dw), torch.zeros_like(dw))
    one = torch.ones_like(cosv)
    pdf_l = torch.where(need_env, env_pdf_t(pmf, dw), torch.zeros_like(cosv))
    pdf_s, pdf_branch = brdf_pdf_t(n, wi, wo, rough)
    if mode == 0:
        w = 1 / torch.where(pdf_l > 0, pdf_l, one)
    elif mode == 1:
        w = inv_pdf
    elif mode == 2:
        s = pdf_s + pdf_l
        w = torch.where(s > 1e-6, 1 / torch.where(s > 1e-6, s, one), torch.zeros_like(s))
    else:
        w = 1 / torch.where(pdf_s > 0, pdf_s, one)
    Li = em * t[:, None] + (ind if ind is not None else 0.0)
    z = torch.zeros_like(em)
    live = ~masked
    Ld = torch.where(live[:, None], Li * diff[:, None] * w[:, None], z)
    Ls = torch.where(live[:, None], Li * spec * w[:, None], z)
    Lo = ((1 - metal[:, None]) * albedo) * Ld + Ls
    vis = (2 * t)[:, None].expand(-1, 3)
    H, W, _ = base.shape
    fp = footprint(dw, H, W)
    py, px = pdf_texel(dw, H, W)
    NoV = (n * wi).sum(-1)
    dec = dict(fp, pdf_y=py, pdf_x=px, masked=masked, need_env=need_env, lit=cosv > 0, front=NoV > 0, pdf_zero=need_env & ~(pdf_l > 0),
               pdf_branch=pdf_branch, mis_on=(pdf_s + pdf_l) > 1e-6, dw=dw.detach())
    return Lo, Ld, Ls, vis, dec


# ---- the generator -----------------------------------------------------------------------------------------------------------
def _orthonormal_to(a, g):
    """a unit vector orthogonal to each (unit) row of a, random azimuth; a draw nearly parallel to its row is replaced by the projection
    of the coordinate axis the row is farthest from."""
    r = torch.randn(a.shape, generator=g, dtype=torch.float64)
    r = r - (r * a).sum(-1, keepdim=True) * a
    e = torch.nn.functional.one_hot(a.abs().argmin(-1), 3).to(a.dtype)
    alt = e - (e * a).sum(-1, keepdim=True) * a
    r = torch.where(r.norm(dim=-1, keepdim=True) < 0.1, alt, r)
    return r / r.norm(dim=-1, keepdim=True)


def _fractions(g, k, side):
    """k fractions from [0.1, 0.4) (side 0) or [0.6, 0.9) (side 1)."""
    return 0.1 + 0.3 * torch.rand(k, generator=g, dtype=torch.float64) + 0.5 * side.double()


def _axis_coords(g, k, size, kind):
    """floor and fraction along one axis of `size` texels.  kind: 'any' (every floor in [-1, size-1]), 'inner' (both neighbours inside),
    'first' (floor -1: clamped row / seam from the left), 'last' (floor size-1), 'edge' (first or last, alternating)."""
    side = torch.randint(0, 2, (k,), generator=g)
    if kind == "any":
        f = torch.randint(-1, size, (k,), generator=g)
    elif kind == "inner":
        f = torch.randint(0, size - 1, (k,), generator=g) if size >= 2 else torch.randint(-1, size, (k,), generator=g)
    elif kind == "first":
        f = torch.full((k,), -1)
    elif kind == "last":
        f = torch.full((k,), size - 1)
    else:
        f = torch.where(torch.arange(k) % 2 == 0, torch.full((k,), -1), torch.full((k,), size - 1))
    side = torch.where(f == -1, torch.ones_like(side), side)                 # u, v >= 0: floor -1 only with a fraction >= 0.5
    side = torch.where(f == size - 1, torch.zeros_like(side), side)          # u, v <= 1
    return f, _fractions(g, k, side)


_ROT = {}


def rotation(seed0=0):
    """w2s[:3,:3]: an orthogonal matrix (fp64 QR, rounded to fp32) whose FIRST ROW -- the world direction of wo = e_x, the NoL == 0 class --
    lies >= 0.01 texel from every footprint / pdf-texel boundary of every map in MAPS (first seed that does)."""
    if seed0 not in _ROT:
        for s in range(seed0, seed0 + 10_000):
            Q, _ = torch.linalg.qr(torch.randn(3, 3, generator=seeded(7919 + s), dtype=torch.float64))
            R = Q.float().contiguous()
            d = R[0:1].double()
            d = d / d.norm()
            if all(float(boundary_distance(d, H, W)) >= 0.01 for H, W in MAPS):
                _ROT[seed0] = R
                break
    return _ROT[seed0]


def make_problem(F, hw, seed, shift=0, indirect=True):
    """fp32 inputs of one shading batch of F rows on an H x W map, built per class (module docstring).  Returns a dict; `lab` holds the
    per-row class names, `target` the (y, x) zero texel a zero_pmf row is aimed at (-1 elsewhere)."""
    H, W = hw
    g = seeded(seed * 1_000_003 + F * 31 + H * 7 + W)
    lab = labels(F, shift)
    R = rotation()
    R64 = R.double()
    base = 0.2 + torch.rand(H, W, 3, generator=g)
    zt = zero_texels(H, W)
    for (y, x) in zt:
        base[y, x] = 0.0
    # ---- world light directions from texel coordinates
    f64 = torch.float64
    x0f, ax = _axis_coords(g, F, W, "any")
    y0f, ay = _axis_coords(g, F, H, "any")
    for kind, xk, yk in (("interior", "inner", "inner"), ("seam", "edge", "inner"), ("top", "any", "first"), ("bottom", "any", "last")):
        m = mask_of(lab["texel"], kind)
        k = int(m.sum())
        if k:
            fx_, ax_ = _axis_coords(g, k, W, xk)
            fy_, ay_ = _axis_coords(g, k, H, yk)
            x0f[m], ax[m], y0f[m], ay[m] = fx_, ax_, fy_, ay_
    target = torch.full((F, 2), -1, dtype=torch.long)
    m = mask_of(lab["texel"], "zero_pmf")
    k = int(m.sum())
    if k:
        if zt:
            which = torch.arange(k) % len(zt)
            ty, tx = torch.tensor([t[0] for t in zt])[which], torch.tensor([t[1] for t in zt])[which]
            sx, sy = torch.randint(0, 2, (k,), generator=g), torch.randint(0, 2, (k,), generator=g)
            # nearest texel = target: floor = target with a low fraction, or target - 1 with a high one
            x0f[m], ax[m] = tx - sx, _fractions(g, k, sx)
            y0f[m], ay[m] = ty - sy, _fractions(g, k, sy)
            target[m] = torch.stack([ty, tx], -1)
        else:                                                           # tiny maps: no zero texel, an interior sample instead
            fx_, ax_ = _axis_coords(g, k, W, "inner")
            fy_, ay_ = _axis_coords(g, k, H, "inner")
            x0f[m], ax[m], y0f[m], ay[m] = fx_, ax_, fy_, ay_
    # next to the poles (theta of a few pi / H) the fp32 rounding of wo moves azimuth and polar angle by ~2^-24 / sin(theta): 0.007 texel in
    # the clamped rows of the 256 x 512 map, 0.001 in the rows beside them.  The fractions of the four rows at either end come from the inner
    # half of each interval, [0.175, 0.325) u [0.675, 0.825)
    polar = (y0f < 3) | (y0f > H - 5)
    inner_half = lambda a: torch.where(polar, torch.where(a < 0.5, 0.25 + 0.5 * (a - 0.25), 0.75 + 0.5 * (a - 0.75)), a)      # noqa: E731
    ax, ay = inner_half(ax), inner_half(ay)
    u = (x0f.to(f64) + ax + 0.5) / W
    v = (y0f.to(f64) + ay + 0.5) / H
    d_world = uv_to_dir(u, v)
    wo = d_world @ R64.T
    wo = wo / wo.norm(dim=-1, keepdim=True)
    # ---- normal and view direction from prescribed cosines
    cos = lab["cos"]
    NoL = 0.02 + 0.96 * torch.rand(F, generator=g, dtype=f64)
    NoV = 0.02 + 0.96 * torch.rand(F, generator=g, dtype=f64)
    NoL = torch.where(mask_of(cos, "nol_neg"), -NoL, NoL)
    NoV = torch.where(mask_of(cos, "nov_neg"), -NoV, NoV)
    close = (NoL + NoV).abs() < 0.02                                      # NoH of the pdf branch: move NoV away from -NoL
    NoV = torch.where(close, torch.sign(NoV) * (NoL.abs() + torch.where(NoL.abs() < 0.5, 0.04, -0.04)), NoV)
    zero = mask_of(cos, "nol_zero")
    wo = torch.where(zero[:, None], torch.tensor([1.0, 0.0, 0.0], dtype=f64), wo)
    e1 = _orthonormal_to(wo, g)
    n = NoL[:, None] * wo + torch.sqrt(1 - NoL ** 2)[:, None] * e1
    n = torch.where(zero[:, None], torch.tensor([0.0, 0.0, 1.0], dtype=f64), n)
    # wi = NoV n + sin (cos psi t1 + sin psi t2), t1 = the part of wo orthogonal to n, |psi| <= 2.4: wi stays away from -wo
    t1 = wo - (wo * n).sum(-1, keepdim=True) * n
    t1 = t1 / t1.norm(dim=-1, keepdim=True)
    t2 = torch.cross(n, t1, dim=-1)
    psi = (torch.rand(F, generator=g, dtype=f64) * 2 - 1) * 2.4
    wi = NoV[:, None] * n + torch.sqrt(1 - NoV ** 2)[:, None] * (torch.cos(psi)[:, None] * t1 + torch.sin(psi)[:, None] * t2)
    # ---- materials, transmittance, weights
    mid = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g)      # noqa: E731
    rough = mid(0.2, 0.9, F)
    for name, val in ROUGH_VALUE.items():
        rough[mask_of(lab["rough"], name)] = val
    metal = mid(0.05, 0.95, F)
    metal[mask_of(lab["metal"], "zero")] = 0.0
    metal[mask_of(lab["metal"], "one")] = 1.0
    albedo = mid(0.05, 0.9, F, 3)
    albedo[mask_of(lab["albedo"], "c0_zero"), 0] = 0.0
    albedo[mask_of(lab["albedo"], "c0_one"), 0] = 1.0
    m = mask_of(lab["albedo"], "c2_zero_c1_one")
    albedo[m, 2], albedo[m, 1] = 0.0, 1.0
    tr = mid(0.05, 0.95, F)
    for name, val in TR_VALUE.items():
        tr[mask_of(lab["tr"], name)] = val
    inv_pdf = 4 * math.pi * mid(0.5, 1.5, F)
    ind = mid(0.0, 0.5, F, 3) if indirect else None
    ups = [torch.randn(F, 3, generator=g) for _ in range(3)]               # g_Lo, g_Lo_diff, g_Lo_spec
    return dict(F=F, hw=hw, lab=lab, target=target, n=n.float(), view_dirs=(-wi).float(), wo=wo.float(), albedo=albedo, rough=rough, metal=metal,
                tr=tr, ind=ind, inv_pdf=inv_pdf, base=base, pmf=env_pmf(base), R=R, ups=ups)


def shade_ref(p, mode, dtype, used=(True, True, True), env_grad=True):
    """forward outputs and autograd of L = sum over the used outputs (Lo, Lo_diff, Lo_spec) of <upstream, output> in `dtype`."""
    mode = MODES.get(mode, mode)
    c = lambda k: None if p[k] is None else p[k].to(dtype)      # noqa: E731
    leaf = lambda k: p[k].to(dtype).clone().requires_grad_(True)      # noqa: E731
    n, albedo, rough, metal = leaf("n"), leaf("albedo"), leaf("rough"), leaf("metal")
    base = leaf("base") if env_grad else c("base")
    Lo, Ld, Ls, vis, dec = shade_t(mode, n, albedo, rough, metal, c("view_dirs"), c("wo"), c("tr"), c("ind"), c("inv_pdf"), base, c("pmf"), c("R"))
    out = dict(Lo=Lo.detach(), Lo_diff=Ld.detach(), Lo_spec=Ls.detach(), vis=vis.detach(), dec=dec)
    if mode <= 1 and any(used):
        L = sum((p["ups"][k].to(dtype) * o).sum() for k, o in enumerate((Lo, Ld, Ls)) if used[k])
        leaves = [n, albedo, rough, metal] + ([base] if env_grad else [])
        g = torch.autograd.grad(L, leaves, allow_unused=True)
        g = [torch.zeros_like(l) if x is None else x for x, l in zip(g, leaves)]
        out.update(g_normal=g[0], g_albedo=g[1], g_roughness=g[2], g_metallic=g[3], g_env=g[4] if env_grad else None)
    return out


def texel_adds(dec, shape):
    """P: the largest number of atomic adds one texel channel receives -- every sample whose environment lookup is live adds to its four
    footprint texels (a clamped row names the same texel twice)."""
    H, W = shape
    live = dec["need_env"]
    idx = torch.cat([(dec[a] * W + dec[b])[live] for a in ("y0", "y1") for b in ("x0", "x1")])
    return int(torch.bincount(idx, minlength=H * W).max()) if idx.numel() else 0


def scatterer_ref(p, lobes, dtype, ups):
    """scatterer.eval of the lobe set and autograd of <g_diff, diff> + <g_spec, spec> w.r.t. (normal, roughness, albedo, metallic)."""
    leaf = lambda k: p[k].to(dtype).clone().requires_grad_(True)      # noqa: E731
    n, albedo, rough, metal = leaf("n"), leaf("albedo"), leaf("rough"), leaf("metal")
    diff, spec = scatterer_eval_t(lobes, n, -p["view_dirs"].to(dtype), p["wo"].to(dtype), rough, albedo, metal)
    L = (ups[0].to(dtype) * diff).sum() + (ups[1].to(dtype) * spec).sum()
    leaves = [n, rough, albedo, metal]
    g = torch.autograd.grad(L, leaves, allow_unused=True)
    g = [torch.zeros_like(l) if x is None else x for x, l in zip(g, leaves)]
    return dict(diff=diff.detach(), spec=spec.detach(), g_normal=g[0], g_roughness=g[1], g_albedo=g[2], g_metallic=g[3])


def row_groups(p):
    """the rows of a batch split by roughness class -- the partition the comparisons run over.  At roughness 0.05 the GGX lobe and its
    derivatives reach 1e2 .. 1e5 where NoH is near 1; compared in one max-norm with the other rows, the fp32 error of those few rows
    would set the tolerance for all of them."""
    return {name: mask_of(p["lab"]["rough"], name) for name in ROUGH}
