"""Plain torch references of the training-backward kernels, their input generators and the comparison rule.

Nothing here touches the GPU or imports the library.  Every reference is ONE formula that runs in whatever dtype its inputs have:
fed the fp32 inputs cast up it is `ref64`, fed the fp32 inputs as they are (on the CPU) it is `twin32`.  The comparison rule
(`compare`) takes its tolerance from the distance between those two, so no tolerance is written down anywhere:

    e32   = max|twin32 - ref64|                  what a straightforward fp32 evaluation loses
    floor = 32 * 2^-23 * max|ref64|              for quantities where the twin happens to round exactly
    assert max|got - ref64| <= max(16 * e32, floor)   and   max|ref64| > 0

The factor 16 covers what separates the kernels from a straightforward fp32 evaluation: another summation order (MFMA tiles,
split-K, float atomics against a sequential sum) and the hardware exp2 / log / __expf in sigmoid and softplus (~2 ulp each).

One derived exception, for the bias gradients (column sums over ALL n rows that every wave adds to one address with a float
atomic): the twin is no sequential sum -- torch's CPU reduction is a cascade (pairwise) sum, whose error stays near one ulp of the
result (e32 ~ 1.5e-7 of it at n = 65 637; a single column can land on 0.1 ulp by chance), while P atomic adds in arbitrary order
are a P-step random walk of roundings, each uniform within +-2^-24 |running sum| (standard deviation 2^-24 |s| / sqrt(3)).  Its
4-sigma radius, 4 * sqrt(P / 3) * 2^-24 * max|ref64|, is allowed on top for those quantities (`atomic_adds=P`, P = number of waves
that contribute: <= 1024 in the fused kernels, <= 3072 in ia_wgrad; 1.5e-5 of the result at P = 3072, nothing at small n).  A lost
row or slab changes such a sum by ~1e-2 of it.  Everything else keeps 16.
"""
import math

import torch
import torch.nn.functional as F

FACTOR = 16.0
FLOOR_ULPS = 32.0
# past every grid cap in rows (fused 256*4*32 = 32 768, operand path 256*4*64 = 65 536, ia_wgrad 768*4*16 = 49 152), so every
# grid-stride loop runs a second iteration; ragged modulo 16, 32 and 64
N_BIG = 65_637

TABLE = []              # (what, err, e32, err / e32) of every comparison of this process, in order


def _d(t):
    return t.detach().cpu().double()


def atomic_radius(atomic_adds, scale):
    return 4.0 * math.sqrt(atomic_adds / 3.0) * 2.0 ** -24 * scale


def compare(what, got, ref64, twin32, factor=FACTOR, atomic_adds=0):
    """the comparison rule; prints and records one table row, then asserts.  atomic_adds: see the module docstring (bias sums only)."""
    got, ref64, twin32 = _d(got), _d(ref64), _d(twin32)
    assert got.shape == ref64.shape == twin32.shape, (what, got.shape, ref64.shape, twin32.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite kernel result"
    scale = float(ref64.abs().max())
    err = float((got - ref64).abs().max())
    e32 = float((twin32 - ref64).abs().max())
    floor = FLOOR_ULPS * 2.0 ** -23 * scale
    ratio = err / e32 if e32 > 0 else math.inf if err > 0 else 0.0
    TABLE.append((what, err, e32, ratio))
    print(f"CMP {what:<44s} err {err:9.3e}  e32 {e32:9.3e}  err/e32 {ratio:8.2f}  max|ref| {scale:9.3e}")
    assert scale > 0.0, f"{what}: vacuous comparison (the reference is all zero)"
    # The third term is non-zero for the bias gradients only (atomic_adds = P waves, one float atomic per wave and column).  Why
    # 16 does not do there: torch's CPU sum (the twin) is pairwise, so 16 * e32 is only about ONE sigma of the P-step random walk
    # of roundings that P atomic adds in arbitrary order are (sigma = sqrt(P / 3) * 2^-24 * |sum|) -- at n = 65 637 the ratio
    # err / e32 of ia_wgrad's db moved between 1.0 and 11.9 in two runs of the same inputs.  Allowed instead: 4 sigma of that walk.
    assert err <= max(factor * e32, floor, atomic_radius(atomic_adds, scale)), (what, err, e32, ratio, floor, atomic_adds)


def fold_table(rows=None):
    """TABLE folded to one row per kernel and quantity: the case with the largest err / e32.  The case parameters (`name=value`
    words and ia_wgrad's `M.. N.. gs.. as..`) are what distinguishes the cases of a quantity; they go into the last column."""
    import re
    best = {}
    for what, err, e32, ratio in (TABLE if rows is None else rows):
        words = what.split()
        is_par = [("=" in w) or bool(re.fullmatch(r"(M|N|gs|as)\d+", w)) for w in words]
        key = " ".join(w for w, par in zip(words, is_par) if not par)
        pars = " ".join(w for w, par in zip(words, is_par) if par) or "-"
        if key not in best or ratio > best[key][2]:
            best[key] = (err, e32, ratio, pars)
    return [(k,) + v for k, v in best.items()]


def format_table(rows=None):
    out = ["%-44s %9s %9s %8s   %s" % ("quantity", "err", "e32", "err/e32", "worst case")]
    out += ["%-44s %9.2e %9.2e %8.2f   %s" % r for r in fold_table(rows)]
    return "\n".join(out)


def seeded(seed):
    return torch.Generator().manual_seed(int(seed))


def randn(g, *shape, scale=0.3):
    return torch.randn(*shape, generator=g) * scale


def up(*ts):
    return [t.double() if (t is not None and t.is_floating_point()) else t for t in ts]


# ----------------------------------------------------------------------------------------------------------------------
# ReLU MLPs with a sigmoid output: kind 1 radiance 67 -> 64 -> 64 -> 3, kind 2 material 48 -> 64 -> 64 -> 5
MLP2_SPEC = {1: ((32, 1.0, 0.0), (3, 2.0, -1.0), (13, 1.0, 0.0), (16, 1.0, 0.0), (3, 1.0, 0.0)),
             2: ((32, 1.0, 0.0), (3, 2.0, -1.0), (13, 1.0, 0.0))}
MLP2_OUT = {1: 3, 2: 5}


def mlp2_in_dim(kind):
    return sum(w for w, _, _ in MLP2_SPEC[kind])


def mlp2_assemble(kind, segs):
    return torch.cat([s * m + a for s, (_, m, a) in zip(segs, MLP2_SPEC[kind])], -1)


def mlp2_forward(kind, segs, W1, b1, W2, b2, W3, b3):
    X = mlp2_assemble(kind, segs)
    z1 = X @ W1.T + b1
    A1 = torch.relu(z1)
    z2 = A1 @ W2.T + b2
    A2 = torch.relu(z2)
    z3 = A2 @ W3.T + b3
    return dict(X=X, z1=z1, A1=A1, z2=z2, A2=A2, z3=z3, y=torch.sigmoid(z3))


def mlp2_ref(kind, prob, dtype):
    """autograd of L = <g_y, y> in `dtype`: gradients of the segments, the assembled row, the pre-activations and the six weights."""
    cast = lambda t: t.to(dtype).clone().requires_grad_(True)      # noqa: E731
    segs = [cast(s) for s in prob["segs"]]
    ws = [cast(w) for w in prob["weights"]]
    f = mlp2_forward(kind, segs, *ws)
    L = (prob["g_y"].to(dtype) * f["y"]).sum()
    inter = [f["X"], f["z1"], f["z2"], f["z3"]]
    g = torch.autograd.grad(L, segs + ws + inter)
    ns = len(segs)
    out = dict(g_segs=list(g[:ns]), g_w=list(g[ns:ns + 6]), g_x=g[ns + 6], G1=g[ns + 7], G2=g[ns + 8], G3=g[ns + 9],
               X=f["X"].detach(), A1=f["A1"].detach(), A2=f["A2"].detach(), y=f["y"].detach())
    return out


def mlp2_bands(kind, segs, weights):
    """fp64 forward and the rigorous fp32 dot-product rounding bounds g1 / g2 of the two hidden pre-activations."""
    segs, (W1, b1, W2, b2, W3, b3) = up(*segs), up(*weights)
    f = mlp2_forward(kind, segs, W1, b1, W2, b2, W3, b3)
    IN = mlp2_in_dim(kind)
    u = 2.0 ** -24
    g1 = (IN + 1) * u * (f["X"].abs() @ W1.abs().T + b1.abs())
    g2 = 65 * u * (f["A1"].abs() @ W2.abs().T + b2.abs()) + g1 @ W2.abs().T
    return f, g1, g2


def mlp2_guard(kind, segs, weights, margin=1.0):
    """rows with a ReLU pre-activation inside (margin x) the rigorous fp32 dot-product rounding bound of 0 (fp64 evaluation)."""
    f, g1, g2 = mlp2_bands(kind, segs, weights)
    return (f["z1"].abs() < margin * g1).any(-1) | (f["z2"].abs() < margin * g2).any(-1)


def make_mlp2_problem(kind, n, seed, zero_units=False, max_rounds=8, cap=0.05):
    """fp32 inputs of one MLP backward (randn * 0.3) without a ReLU pre-activation within rounding distance of 0: such rows are
    redrawn (deterministically, at most `max_rounds` times); the first round may touch at most `cap` of the rows.
    zero_units: W1[5,:] = b1[5] = 0 and W2[7,:] = b2[7] = 0 -- those pre-activations are EXACTLY 0 in every row (gradient 0)."""
    g = seeded(seed)
    widths = [w for w, _, _ in MLP2_SPEC[kind]]
    IN, OUT = mlp2_in_dim(kind), MLP2_OUT[kind]
    segs = [randn(g, n, w) for w in widths]
    weights = [randn(g, 64, IN), randn(g, 64), randn(g, 64, 64), randn(g, 64), randn(g, OUT, 64), randn(g, OUT)]
    if zero_units:
        weights[0][5, :] = 0.0; weights[1][5] = 0.0
        weights[2][7, :] = 0.0; weights[3][7] = 0.0
    g_y = randn(g, n, OUT)
    first = None
    for rnd in range(max_rounds + 1):
        bad = mlp2_guard(kind, segs, weights)
        nb = int(bad.sum())
        if first is None:
            first = nb
        if nb == 0:
            break
        assert rnd < max_rounds, f"rows inside the ReLU guard band after {max_rounds} rounds: {nb}"
        gr = seeded(seed * 1000 + 17 + rnd)
        for s, w in zip(segs, widths):
            s[bad] = randn(gr, n, w)[bad]
    assert first <= cap * n, f"kind {kind} n {n} seed {seed}: first round redrew {first} of {n} rows (cap {cap:.0%})"
    return dict(kind=kind, n=n, segs=segs, weights=weights, g_y=g_y, first_round_redrawn=first)


# seeds of the (kind, n) cases of the GPU file (tiny n: seeds whose first round stays under the 5 % cap)
MLP2_NS = (1, 31, 32, 33, 63, 64, 65, 257, N_BIG)
MLP2_OPERAND_NS = (63, 65, N_BIG)
MLP2_SEED = {(1, 1): 1, (1, 31): 1, (1, 32): 1, (1, 33): 1, (1, 63): 1, (1, 64): 1, (1, 65): 1, (1, 257): 1, (1, N_BIG): 1,
             (2, 1): 1, (2, 31): 1, (2, 32): 1, (2, 33): 1, (2, 63): 1, (2, 64): 1, (2, 65): 1, (2, 257): 1, (2, N_BIG): 1}
MLP2_ZERO_CASE = (257, 3)        # (n, seed) of the exact-zero ReLU case, both kinds


# ----------------------------------------------------------------------------------------------------------------------
# SDF head 35 -> 64 -> 13, Softplus(beta = 100), with the second-order path through the analytic normal
SDF_NS = (1, 31, 33, 64, 65, N_BIG)
SDF_OPERAND_NS = (65, N_BIG)
SDF_SEED = 1
SDF_W1_SCALE = 0.045           # z = h W1^T + b1 then has a standard deviation of ~0.12: most units inside the softplus knee


def make_sdf_problem(n, seed):
    g = seeded(seed)
    p = dict(n=n, enc=randn(g, n, 32), xyz=randn(g, n, 3), jac=randn(g, n, 32, 3),
             W1=randn(g, 64, 35, scale=SDF_W1_SCALE), b1=randn(g, 64, scale=SDF_W1_SCALE), W2=randn(g, 13, 64), b2=randn(g, 13),
             g_out=randn(g, n, 13), q=randn(g, n, 3))
    return p


def sdf_regime_shares(p):
    """(share of (row, unit) pairs with |100 z| < 10, share with 100 z > 20) in fp64."""
    h = torch.cat([p["enc"].double(), 2.0 * p["xyz"].double() - 1.0], -1)
    bz = 100.0 * (h @ p["W1"].double().T + p["b1"].double())
    return float((bz.abs() < 10).double().mean()), float((bz > 20).double().mean())


def sdf_ref(p, dtype):
    """double backward: L = <g_out, out> + <q, d out[:,0].sum() / d x>; everything the SDF backward kernels emit."""
    c = lambda k: p[k].to(dtype).clone().requires_grad_(True)      # noqa: E731
    enc0, J, x, W1, b1, W2, b2 = c("enc"), c("jac"), c("xyz"), c("W1"), c("b1"), c("W2"), c("b2")
    g_out, q = p["g_out"].to(dtype), p["q"].to(dtype)
    x0 = x.detach()
    h = torch.cat([enc0 + torch.einsum("nkc,nc->nk", J, x - x0), 2.0 * x - 1.0], -1)
    out = F.softplus(h @ W1.T + b1, beta=100) @ W2.T + b2
    sdf_sum = out[:, 0].sum()
    grad, = torch.autograd.grad(sdf_sum, x, create_graph=True)
    gG, = torch.autograd.grad(sdf_sum, enc0, retain_graph=True)
    L = (g_out * out).sum() + (q * grad).sum()
    gE, gJ, gx, dW1, db1, dWo, dbo = torch.autograd.grad(L, [enc0, J, x, W1, b1, W2, b2])
    return dict(gE=gE, gG=gG, gJ=gJ, gx=gx, dW1=dW1, db1=db1, dWo=dWo, dbo=dbo, grad=grad.detach(), out=out.detach())


def sdf_closed_form(p, dtype=torch.float64):
    """second opinion only (the derivation the kernels implement), checked against sdf_ref on the CPU."""
    enc, xyz, J, W1, b1, W2, b2, g_out, q = (p[k].to(dtype) for k in ("enc", "xyz", "jac", "W1", "b1", "W2", "b2", "g_out", "q"))
    h = torch.cat([enc, 2.0 * xyz - 1.0], -1)
    z = h @ W1.T + b1
    s = torch.sigmoid(100.0 * z)
    a = F.softplus(z, beta=100)
    gz = s * W2[0]
    gh = gz @ W1
    u = torch.cat([torch.einsum("nkc,nc->nk", J, q), 2.0 * q], -1)
    dgz = u @ W1.T
    da = g_out @ W2
    dz = da * s + dgz * W2[0] * 100.0 * s * (1.0 - s)
    dh = dz @ W1
    dWo = g_out.T @ a
    dWo[0] += (dgz * s).sum(0)
    return dict(gE=dh[:, :32], gG=gh[:, :32], g_xyz=dh[:, 32:35], dW1=dz.T @ h + gz.T @ u, db1=dz.sum(0), dWo=dWo, dbo=g_out.sum(0),
                gx=torch.einsum("nkc,nk->nc", J, dh[:, :32]) + 2.0 * dh[:, 32:35])


# ----------------------------------------------------------------------------------------------------------------------
# split-K weight gradient
WGRAD_NS = (1, 15, 16, 17, N_BIG)
WGRAD_SHAPES = ((64, 67, 64, 68), (64, 64, 64, 64), (3, 64, 16, 64), (64, 35, 64, 36), (13, 64, 13, 64), (64, 1, 64, 64),
                (1, 96, 4, 96), (64, 96, 64, 96))        # (M, N, g_stride, a_stride); (64, 1, 64, 64): A is G itself


def make_wgrad_problem(n, shape, seed, garbage=0.0):
    """G [n, g_stride], A [n, a_stride] with columns >= M / >= N set to `garbage`."""
    M, N, gs, as_ = shape
    g = seeded(seed)
    G = randn(g, n, gs)
    G[:, M:] = garbage
    if shape == (64, 1, 64, 64):
        return G, G
    A = randn(g, n, as_)
    A[:, N:] = garbage
    return G, A


def wgrad_ref(G, M, A, N, dtype):
    G, A = G.to(dtype), A.to(dtype)
    return G[:, :M].T @ A[:, :N], G[:, :M].sum(0)


# ----------------------------------------------------------------------------------------------------------------------
# shading prep: normals and the reflected view direction
def make_shade_prep_problem(n, seed):
    """sdf_grad rows: |g| >= 1e-3 except two families -- exact zeros, and |g| in [1e-9, 1e-7] (the clamped branch of
    x / max(|x|, 1e-6)); ray_indices unsorted with repeats."""
    g = seeded(seed)
    n_rays = max(1, n // 3)
    sdf_grad = randn(g, n, 3, scale=1.0)
    nrm = sdf_grad.norm(dim=-1, keepdim=True)
    sdf_grad = sdf_grad / nrm * (nrm + 1e-3)                         # every ordinary row has |g| >= 1e-3
    if n >= 8:
        sdf_grad[1::16] = 0.0
        k = sdf_grad[3::16].shape[0]
        d = F.normalize(randn(g, k, 3, scale=1.0), dim=-1)
        sdf_grad[3::16] = d * (10.0 ** (-9.0 + 2.0 * torch.rand(k, 1, generator=g)))
    rays_d = F.normalize(randn(g, n_rays, 3, scale=1.0), dim=-1) * (0.5 + torch.rand(n_rays, 1, generator=g))
    ray_indices = torch.randint(0, n_rays, (n,), generator=g)
    Q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g).double())
    R = Q.float().contiguous()
    ups = [randn(g, n, 3, scale=1.0) for _ in range(3)]             # g_ns, g_nw, g_rf
    return dict(n=n, sdf_grad=sdf_grad, rays_d=rays_d, ray_indices=ray_indices, R=R, ups=ups)


def shade_prep_forward(sdf_grad, rays_d, ray_indices, R):
    nw = F.normalize(sdf_grad @ R, dim=-1, eps=1e-6)
    vw = F.normalize(rays_d[ray_indices] @ R, dim=-1, eps=1e-6)
    ns = F.normalize(sdf_grad, dim=-1, eps=1e-6)
    dt = -(vw * nw).sum(-1, keepdim=True)
    rf = ((2.0 * dt * nw + vw) + 1.0) / 2.0
    return ns, nw, rf


def shade_prep_ref(p, used, dtype):
    """d / d sdf_grad of sum over the used outputs (ns, nw, rf) of <upstream, output>."""
    sg = p["sdf_grad"].to(dtype).clone().requires_grad_(True)
    outs = shade_prep_forward(sg, p["rays_d"].to(dtype), p["ray_indices"], p["R"].to(dtype))
    L = sum((p["ups"][k].to(dtype) * outs[k]).sum() for k in range(3) if used[k])
    return torch.autograd.grad(L, sg)[0], [o.detach() for o in outs]


# ----------------------------------------------------------------------------------------------------------------------
# select + push-forward
def make_select_push_problem(n, seed):
    g = seeded(seed)
    P = 2 * n + 3
    valid = torch.rand(n, generator=g) > 0.3
    sel = torch.randint(0, n, (n,), generator=g, dtype=torch.int32)
    if n > 1:
        valid[0], valid[1] = True, False
        sel[~valid] = -1
        sel[1::7] = -1
    else:
        valid[0] = True
    cand_src = torch.randint(0, P, (n,), generator=g, dtype=torch.int32)
    return dict(n=n, out=randn(g, n, 13), grad_c=randn(g, n, 3), valid=valid, fwd_J=randn(g, P, 9, scale=1.0), cand_src=cand_src,
                sel=sel, ups=[randn(g, n, 13), randn(g, n), randn(g, n, 3)])


def select_push_forward(out, grad_c, valid, fwd_J, cand_src, sel):
    n = out.shape[0]
    if fwd_J is None:
        c2w = torch.zeros((n, 3, 3), dtype=out.dtype)
    else:
        c2w = fwd_J.reshape(-1, 3, 3)[cand_src.long()[sel.long().clamp(min=0)]]
    feat = torch.where(valid[:, None], out, torch.zeros_like(out))
    sdf = torch.where(valid, out[:, 0], torch.full_like(out[:, 0], 1e5))
    dflt = torch.tensor([0.0, 0.0, 1.0], dtype=out.dtype)
    sdf_grad = torch.where(valid[:, None], (c2w * grad_c[:, None, :]).sum(-1), dflt[None])
    return feat, sdf, sdf_grad, c2w


def select_push_ref(p, used, with_J, dtype):
    out = p["out"].to(dtype).clone().requires_grad_(True)
    gc = p["grad_c"].to(dtype).clone().requires_grad_(True)
    J = p["fwd_J"].to(dtype) if with_J else None
    outs = select_push_forward(out, gc, p["valid"], J, p["cand_src"], p["sel"])
    L = sum((p["ups"][k].to(dtype) * outs[k]).sum() for k in range(3) if used[k])
    g_out, g_gc = torch.autograd.grad(L, [out, gc], allow_unused=True)
    z = torch.zeros_like
    return (g_out if g_out is not None else z(out)), (g_gc if g_gc is not None else z(gc)), [o.detach() for o in outs]


# ----------------------------------------------------------------------------------------------------------------------
# eikonal term
EIKONAL_NS = (0, 1, 1023, 1024, 1025, 4099)


def make_eikonal_problem(n, seed, all_invalid=False):
    g = seeded(seed)
    sdf_grad = randn(g, n, 3, scale=0.7)
    valid = torch.rand(n, generator=g) > 0.25
    if n > 0:
        valid[0] = True
    if n > 4:
        sdf_grad[2] = 0.0                  # a zero-norm VALID row: gradient 0
        valid[2] = True
        valid[3] = False
    if all_invalid:
        valid[:] = False
    return dict(n=n, sdf_grad=sdf_grad, valid=valid)


def eikonal_ref(p, w, dtype):
    """(sum over valid of (|g| - 1)^2, count, d (w * sum) / d g)."""
    sg = p["sdf_grad"].to(dtype).clone().requires_grad_(True)
    v = p["valid"]
    nrm = torch.linalg.norm(sg, dim=-1)
    s = (((nrm - 1.0) ** 2) * v.to(dtype)).sum()
    grad = torch.autograd.grad(s * w, sg)[0] if p["n"] > 0 else torch.zeros_like(sg)
    return s.detach(), float(v.sum()), grad


# ----------------------------------------------------------------------------------------------------------------------
# Laplace density -> alpha
def make_alpha_problem(n, beta, seed):
    g = seeded(seed)
    sdf = randn(g, n, scale=3.0 * beta)
    sdf[0], sdf[1], sdf[2], sdf[3], sdf[4] = 0.0, 1e-30, -1e-30, 200.0 * beta, -200.0 * beta
    dists = 0.01 + 0.05 * torch.rand(n, generator=g)
    return dict(n=n, sdf=sdf, dists=dists, beta=torch.tensor(float(beta)), g_alpha=randn(g, n, scale=1.0))


def alpha_forward(sdf, dists, beta):
    dens = (1.0 / beta) * (0.5 + 0.5 * torch.sign(sdf) * torch.expm1(-sdf.abs() / beta))
    return 1.0 - torch.exp(-dens * dists)


def alpha_ref(p, dtype):
    sdf = p["sdf"].to(dtype).clone().requires_grad_(True)
    beta = p["beta"].to(dtype).clone().requires_grad_(True)
    a = alpha_forward(sdf, p["dists"].to(dtype), beta)
    g_sdf, g_beta = torch.autograd.grad((p["g_alpha"].to(dtype) * a).sum(), [sdf, beta])
    return g_sdf, g_beta, a.detach()


# ----------------------------------------------------------------------------------------------------------------------
# SphericalHarmonics(degree 4) of 2 d01 - 1
def sh4(d01):
    x, y, z = (d01 * 2.0 - 1.0).unbind(-1)
    x2, y2, z2 = x * x, y * y, z * z
    return torch.stack([
        torch.full_like(x, 0.28209479177387814),
        -0.48860251190291987 * y,
        0.48860251190291987 * z,
        -0.48860251190291987 * x,
        1.0925484305920792 * x * y,
        -1.0925484305920792 * y * z,
        0.94617469575755997 * z2 - 0.31539156525251999,
        -1.0925484305920792 * x * z,
        0.54627421529603959 * (x2 - y2),
        0.59004358992664352 * y * (y2 - 3.0 * x2),
        2.8906114426405538 * x * y * z,
        0.45704579946446572 * y * (1.0 - 5.0 * z2),
        0.3731763325901154 * z * (5.0 * z2 - 3.0),
        0.45704579946446572 * x * (1.0 - 5.0 * z2),
        1.4453057213202769 * z * (x2 - y2),
        0.59004358992664352 * x * (3.0 * y2 - x2)], -1)


def make_sh4_problem(n, seed):
    g = seeded(seed)
    d01 = torch.rand(n, 3, generator=g)
    corners = torch.tensor([[a, b, c] for a in (0.0, 1.0) for b in (0.0, 1.0) for c in (0.0, 1.0)] + [[0.5, 0.5, 0.5]]
                           + [[0.5, 0.0, 1.0], [1.0, 0.5, 0.0], [0.0, 1.0, 0.5]])
    k = min(n, corners.shape[0])
    if n >= corners.shape[0]:
        d01[:k] = corners
    else:
        d01[:k] = corners[-k:] if n > 1 else corners[8:9]         # n = 1: the centre row
    return dict(n=n, d01=d01, g_sh=randn(g, n, 16, scale=1.0))


def sh4_ref(p, dtype):
    d = p["d01"].to(dtype).clone().requires_grad_(True)
    return torch.autograd.grad((p["g_sh"].to(dtype) * sh4(d)).sum(), d)[0]


RADIANCE_CASE = (257, 21)            # (n, seed) of the train._Radiance route test
RADIANCE_MARGIN = 2.0


def make_radiance_problem(n, seed, enc_fn, max_rounds=8, cap=0.05):
    """inputs of train._Radiance past its hash grid.  enc_fn(x [n,3] in [0,1)) -> (enc [n,32], xp [n,3]) supplies what the hash-grid
    kernel and the point normalisation produce (on the CPU check: a stand-in of the same magnitude).  The ReLU repair of
    make_mlp2_problem again, with two differences: only `feat` can be redrawn (enc follows x, the SH values follow refl01), and the
    band is RADIANCE_MARGIN x wider, because the SH values the kernel feeds the MLP are an fp32 intermediate, not an input shared
    with the reference.  That the extra band covers it is asserted: 4 x the effect of the fp32 SH error on z1 stays inside
    (margin - 1) x g1 for every (row, unit).  Same 5 % first-round cap."""
    g = seeded(seed)
    p0 = make_mlp2_problem(1, n, seed=1)
    x = torch.rand(n, 3, generator=g)
    enc, xp = enc_fn(x)
    p = dict(n=n, x=x, enc=enc, xp=xp, feat=p0["segs"][2], nrm=p0["segs"][4], refl01=torch.rand(n, 3, generator=g),
             weights=p0["weights"], g_rgb=p0["g_y"])
    sh64 = sh4(p["refl01"].double())
    sh32 = sh4(p["refl01"]).double()
    first = None
    for rnd in range(max_rounds + 1):
        segs = [p["enc"], p["xp"], p["feat"], sh64.float(), p["nrm"]]
        f, g1, g2 = mlp2_bands(1, segs, p["weights"])
        dz1 = (sh32 - sh64).abs() @ p["weights"][0].double()[:, 48:64].abs().T
        assert bool((4.0 * dz1 <= (RADIANCE_MARGIN - 1.0) * g1).all()), "the fp32 SH error is not covered by the widened band"
        bad = (f["z1"].abs() < RADIANCE_MARGIN * g1).any(-1) | (f["z2"].abs() < RADIANCE_MARGIN * g2).any(-1)
        nb = int(bad.sum())
        if first is None:
            first = nb
        if nb == 0:
            break
        assert rnd < max_rounds, f"rows inside the ReLU guard band after {max_rounds} rounds: {nb}"
        p["feat"][bad] = randn(g, n, 13)[bad]
    assert first <= cap * n, f"radiance problem: first round redrew {first} of {n} rows (cap {cap:.0%})"
    p["first_round_redrawn"] = first
    return p


def radiance_ref(p, dtype):
    """train._Radiance past its hash grid: rgb = MLP kind 1 (enc, xp, feat, SH4(refl01), normal), L = <g_rgb, rgb>; gradients of
    (feat, refl01, normal) and the six weights.  enc / xp are inputs (what the hash-grid kernel and the normalisation produced)."""
    c = lambda t: t.to(dtype).clone().requires_grad_(True)      # noqa: E731
    feat, refl01, nrm = c(p["feat"]), c(p["refl01"]), c(p["nrm"])
    ws = [c(w) for w in p["weights"]]
    f = mlp2_forward(1, [p["enc"].to(dtype), p["xp"].to(dtype), feat, sh4(refl01), nrm], *ws)
    g = torch.autograd.grad((p["g_rgb"].to(dtype) * f["y"]).sum(), [feat, refl01, nrm] + ws)
    return dict(rgb=f["y"].detach(), g_feat=g[0], g_refl01=g[1], g_nrm=g[2], g_w=list(g[3:]))


# ----------------------------------------------------------------------------------------------------------------------
# contractions with the stored hash-grid Jacobian
def jac_contract_ref(mode, jac, v, dtype):
    jac, v = jac.to(dtype), v.to(dtype)
    if mode == 0:
        return torch.einsum("nkc,nk->nc", jac, v)
    return torch.einsum("nkc,nc->nk", jac, v)


# ----------------------------------------------------------------------------------------------------------------------
# volume interaction: backward of the per-interval gathers
VI_GATHER_SS = (1, 63, 64, 65, 200)
VI_COUNTS = (0, 1, 2, 63, 64, 65, 200)


def make_vi_gather_problem(S, seed):
    """fg_cnt [S] from VI_COUNTS (so some segments exceed a wave), fg_off = exclusive scan; for S >= 128 the second group of 64
    intervals is all zero."""
    g = seeded(seed)
    cnt = torch.tensor(VI_COUNTS)[torch.randint(0, len(VI_COUNTS), (S,), generator=g)]
    if S == 1:
        cnt[0] = 200
    else:
        cnt[0], cnt[S - 1] = 65, 1
    if S >= 128:
        cnt[64:128] = 0
    cnt = cnt.int()
    off = (torch.cumsum(cnt, 0) - cnt).int()
    Fn = int(cnt.sum())
    ups = [randn(g, Fn, 3, scale=1.0), randn(g, Fn, 3, scale=1.0), randn(g, Fn, scale=1.0), randn(g, Fn, scale=1.0),
           randn(g, Fn, scale=1.0)]            # g_normals_fg, g_albedo_fg, g_roughness_fg, g_metallic_fg, g_weights_fg
    return dict(S=S, F=Fn, cnt=cnt, off=off, ups=ups)


def make_vi_gather_fwd_problem(seed, n_rays=70, spp=128):
    """the composite layout (make_vi_composite_problem) with what ia_vi_gather reads on top: every ray with foreground re-samples
    owns a run of consecutive source intervals; its foreground re-samples name them in non-decreasing order (sampled_idx), so
    the re-samples of interval s are the range [fg_off[s], fg_off[s] + fg_counts[s]) of the ray-major foreground list.  Some
    intervals are never sampled (count 0); background re-samples carry an index that must not be read as foreground."""
    c = make_vi_composite_problem(seed, n_rays, spp)
    g = seeded(seed + 1000)
    R = int(c["rpi"][:, 1].sum())
    sidx = torch.zeros(R, dtype=torch.int64)
    counts, s0 = [], 0
    for r in range(n_rays):
        nf, base = int(c["fg_ray_cnt"][r]), int(c["rpi"][r, 0])
        m = 1 + int(torch.randint(0, 6, (1,), generator=g))                  # intervals of this ray (some stay unsampled)
        if int(c["rpi"][r, 1]) > 0:
            pick = torch.sort(torch.randint(0, m, (nf,), generator=g))[0]
            sidx[base:base + nf] = s0 + pick
            sidx[base + nf:base + spp] = s0 + m - 1                           # background tail: not a foreground re-sample
            counts += torch.bincount(pick, minlength=m).tolist()
        else:
            counts += [0] * m
        s0 += m
    S = s0
    fg_cnt = torch.tensor(counts, dtype=torch.int32)
    c.update(S=S, R=R, sidx=sidx, fg_cnt=fg_cnt, fg_off=(torch.cumsum(fg_cnt, 0) - fg_cnt).int(), ts=torch.rand(R, generator=g) * 4.0,
             weights=torch.rand(S, generator=g), rays_o=randn(g, n_rays, 3, scale=1.0), rays_d=randn(g, n_rays, 3, scale=1.0),
             normals=randn(g, S, 3, scale=1.0), albedo=torch.rand(S, 3, generator=g), rough=torch.rand(S, generator=g),
             metal=torch.rand(S, generator=g))
    return c


def vi_gather_fwd_ref(p, dtype):
    """what ia_vi_gather writes, from the layout alone: (fg_src, fg_ray, positions, view_dirs, normals, albedo, roughness, metallic,
    weights / count) over the ray-major foreground list."""
    idx = torch.cat([torch.arange(int(p["fg_ray_cnt"][r])) + int(p["rpi"][r, 0]) for r in range(p["n_rays"])]).long()
    src, ray = p["sidx"][idx], p["fg_ray"].long()
    o, d, t = p["rays_o"].to(dtype)[ray], p["rays_d"].to(dtype)[ray], p["ts"].to(dtype)[idx]
    return dict(fg_src=src.int(), fg_ray=p["fg_ray"], positions=o + d * t[:, None], view_dirs=p["rays_d"][ray], normals=p["normals"][src],
                albedo=p["albedo"][src], rough=p["rough"][src], metal=p["metal"][src],
                weights=p["weights"].to(dtype)[src] / p["fg_cnt"][src].to(dtype))


def vi_gather_bwd_ref(p, present, dtype):
    """index_add of the upstream gradients over each interval's range; the weight gradient is the MEAN over it (0 when empty)."""
    S, cnt = p["S"], p["cnt"].long()
    src = torch.repeat_interleave(torch.arange(S), cnt)
    outs = []
    for k, u in enumerate(p["ups"]):
        shape = (S,) + tuple(u.shape[1:])
        o = torch.zeros(shape, dtype=dtype)
        if present[k]:
            o.index_add_(0, src, u.to(dtype))
        if k == 4:
            o = torch.where(cnt > 0, o / cnt.clamp(min=1).to(dtype), torch.zeros_like(o))
        outs.append(o)
    return outs


# ----------------------------------------------------------------------------------------------------------------------
# volume interaction: composite
def make_vi_composite_problem(seed, n_rays=70, spp=128):
    """a layout that honours the contract of the re-sampler: every ray WITH samples owns spp consecutive re-samples (packed info
    (start, spp)), the first spp - bg_cnt of them foreground; rays without samples have (start, 0).  Foreground counts include
    0 (with samples, all background), 1, 64, 65 and 128 (= spp: bg_cnt 0, transmittance ignored)."""
    g = seeded(seed)
    fg_choices = torch.tensor([0, 1, 64, 65, 128, 7, 100])
    has = torch.rand(n_rays, generator=g) > 0.2
    has[:8] = torch.tensor([True, False, True, True, True, True, True, False])
    nf = fg_choices[torch.randint(0, len(fg_choices), (n_rays,), generator=g)]
    nf[:8] = torch.tensor([1, 0, 64, 65, 128, 0, 100, 0])
    nf = torch.where(has, nf, torch.zeros_like(nf))
    cnt = torch.where(has, torch.full_like(nf, spp), torch.zeros_like(nf))
    start = torch.cumsum(cnt, 0) - cnt
    rpi = torch.stack([start, cnt], -1).int().contiguous()
    bg_cnt = torch.where(has, spp - nf, torch.zeros_like(nf)).int()
    bg_cnt[~has] = torch.randint(0, spp, (int((~has).sum()),), generator=g).int()      # unspecified for rays without samples
    fg_ray_cnt = nf.int()
    fg_start = (torch.cumsum(nf, 0) - nf).int()
    Fn = int(nf.sum())
    fg_ray = torch.repeat_interleave(torch.arange(n_rays), nf).int()
    return dict(n_rays=n_rays, spp=spp, F=Fn, rpi=rpi, bg_cnt=bg_cnt, fg_ray_cnt=fg_ray_cnt, fg_start=fg_start, fg_ray=fg_ray,
                w=torch.rand(Fn, generator=g) / spp, Lo=torch.rand(Fn, 3, generator=g) * 2.0, T=torch.rand(n_rays, generator=g),
                bg=torch.tensor([0.2, 0.4, 0.6]), bg_rays=torch.rand(n_rays, 3, generator=g), g_rgb=randn(g, n_rays, 3, scale=1.0))


def vi_composite_ref(p, with_bg_rays, dtype):
    """per-ray loop; returns rgb and the gradients of <g_rgb, rgb> w.r.t. (w, Lo, T)."""
    w = p["w"].to(dtype).clone().requires_grad_(True)
    Lo = p["Lo"].to(dtype).clone().requires_grad_(True)
    T = p["T"].to(dtype).clone().requires_grad_(True)
    bg, bg_rays = p["bg"].to(dtype), p["bg_rays"].to(dtype)
    rows = []
    for r in range(p["n_rays"]):
        b = bg_rays[r] if with_bg_rays else bg
        if int(p["rpi"][r, 1]) <= 0:
            rows.append(b + 0.0 * T[r])
            continue
        fs, nf = int(p["fg_start"][r]), int(p["fg_ray_cnt"][r])
        c = (w[fs:fs + nf, None] * Lo[fs:fs + nf]).sum(0)
        if int(p["bg_cnt"][r]) > 0:
            c = c + T[r] * b
        rows.append(c)
    rgb = torch.stack(rows)
    g_w, g_Lo, g_T = torch.autograd.grad((p["g_rgb"].to(dtype) * rgb).sum(), [w, Lo, T], allow_unused=True)
    if g_T is None:
        g_T = torch.zeros_like(T)
    return rgb.detach(), g_w, g_Lo, g_T
