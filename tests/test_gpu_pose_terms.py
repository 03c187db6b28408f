"""GPU: the fused pose-term backward (csrc/pose_terms.hip, ia_pose_terms_bwd), its autograd node (deformer._PoseTerms) and the wiring
of the node into train.shade_front for both training dicts.

References and bars
  want      fp64 CPU autograd through the expressions of SNARFDeformer.implicit_pose_terms + `c2w + (R - R.detach()) * valid`, restated
            below (pose_terms_fp64); only the weights are taken from the device (dfm.query_weights, cast to fp64).
  parent    the same expressions in fp32 on the GPU (implicit_pose_terms itself: weights kernel, library product, ATen chain).
  bar       max |kernel - want| <= 2 x max |parent - want|: the kernel may not be worse than the route it replaces; the factor 2 allows
            for another summation order.
  ceiling   per entry, |kernel - want| <= (P + 64) 2^-24 sum_p |w_p[j] G_p|: the worst case of ANY fp32 summation order of P terms
            (P roundings of the running sum) plus 64 roundings for forming G and the weights' own error.  The smoothed weight
            grid holds weights down to 1e-38: where an entry of the result is a subnormal fp32 number its rounding is absolute,
            half a spacing of 2^-149, not relative -- the ceiling carries that one spacing as a floor.
Observed on the MI355X (tools/pose_terms_bench.py -> profiles/pose_terms.json): the kernel's error is the final fp32 rounding.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 63, 65, 257, 4099)


@pytest.fixture(scope="module")
def frame():
    """the tiny frame of tests/test_gpu_fit.py's builder: (rs, rays)"""
    from intrinsicavatar_amd import build
    build.build()
    from intrinsicavatar_amd import synthetic as S
    rs, rays, _ = S.build_frame(DEV, 16, 16, pose_seed=0, beta=0.01, num_samples_per_ray=64, grid_D=16, grid_H=64, grid_W=64, smooth_iters=5,
                                hash_amp=2e-3)
    return rs, rays


@pytest.fixture(scope="module")
def dfm(frame):
    return frame[0].deformer


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


def make_case(dfm, P, seed=0, invalid=0.3):
    """xc over 1.4 x the weight grid's box (the border clamp is hit), random J_inv and gradients, ~30 % invalid points"""
    g = torch.Generator().manual_seed(1000 * seed + P)
    lo, hi = dfm.bbox[0].cpu(), dfm.bbox[1].cpu()
    xc = (lo + hi) / 2 + (torch.rand((P, 3), generator=g) - 0.5) * 1.4 * (hi - lo)
    J_inv = torch.randn((P, 3, 3), generator=g)
    valid = torch.rand(P, generator=g) >= invalid
    if P == 1:
        valid[:] = True                                   # (one point: keep the case from being empty)
    g_pts, g_c2w = torch.randn((P, 3), generator=g), torch.randn((P, 3, 3), generator=g)
    c2w = torch.randn((P, 3, 3), generator=g)
    return {k: v.to(DEV) for k, v in dict(xc=xc.float(), J_inv=J_inv, valid=valid, g_pts=g_pts, g_c2w=g_c2w, c2w=c2w).items()}


def pose_terms_fp64(w, tfs, xc, J_inv, valid, c2w):
    """implicit_pose_terms + the c2w line, restated: w [P,24], tfs [24,4,4] (the leaf), all fp64 on the CPU -> (pts_cano, c2w)"""
    T = (w @ tfs.reshape(24, 16)).reshape(-1, 4, 4)
    R = T[:, :3, :3]
    xd = (R * xc[:, None, :]).sum(-1) + T[:, :3, 3]
    corr = -(J_inv * (xd - xd.detach())[:, None, :]).sum(-1) * valid[:, None]
    return xc + corr, c2w + (R - R.detach()) * valid[:, None, None]


def want_and_ceiling(dfm, c):
    """(want [24,4,4] fp64, ceiling [24,4,4]) for a case"""
    D = lambda t: t.detach().cpu().double()      # noqa: E731
    P = c["xc"].shape[0]
    w = D(dfm.query_weights(c["xc"])) if P else torch.zeros((0, 24), dtype=torch.float64)
    tfs = D(dfm.tfs[0]).requires_grad_(True)
    xc, J_inv, valid = D(c["xc"]), D(c["J_inv"]), D(c["valid"])
    pts, c2w = pose_terms_fp64(w, tfs, xc, J_inv, valid, D(c["c2w"]))
    torch.autograd.backward([pts, c2w], [D(c["g_pts"]), D(c["g_c2w"])])
    gx = -torch.einsum("prc,pr->pc", J_inv, D(c["g_pts"])) * valid[:, None]
    G = torch.cat([D(c["g_c2w"]) * valid[:, None, None] + gx[:, :, None] * xc[:, None, :], gx[:, :, None]], -1)      # [P,3,4]
    ceil = torch.zeros((24, 4, 4), dtype=torch.float64)
    ceil[:, :3, :] = (P + 64) * 2.0 ** -24 * torch.einsum("pj,pre->jre", w.abs(), G.abs()) + 2.0 ** -149
    return tfs.grad, ceil


def parent_route(dfm, c):
    """tfs.grad [24,4,4] of the fp32 torch expressions on the GPU"""
    tfs0 = dfm.tfs
    try:
        dfm.tfs = tfs0.detach().clone().requires_grad_(True)
        pts, R = dfm.implicit_pose_terms(c["xc"], c["J_inv"], c["valid"])
        c2w = c["c2w"] + (R - R.detach()) * c["valid"][:, None, None].to(R.dtype)
        torch.autograd.backward([pts, c2w], [c["g_pts"], c["g_c2w"]])
        return dfm.tfs.grad[0].detach().clone()
    finally:
        dfm.tfs = tfs0


def kernel(dfm, c, win=None, J_inv=None):
    return dfm.pose_terms_backward(c["xc"], c["J_inv"] if J_inv is None else J_inv, c["valid"], c["g_pts"], c["g_c2w"], win)


@pytest.mark.parametrize("P", SIZES)
def test_kernel_against_fp64(dfm, P):
    c = make_case(dfm, P)
    want, ceil = want_and_ceiling(dfm, c)
    err_parent = float((parent_route(dfm, c).cpu().double() - want).abs().max())
    got = kernel(dfm, c).cpu().double()
    err = (got - want).abs()
    print(f"P={P}: kernel max abs error {float(err.max()):.3e}, parent route {err_parent:.3e}, largest entry {float(want.abs().max()):.3e}")
    assert float(want.abs().max()) > 0
    assert bool((err <= ceil).all()), (P, float((err - ceil).max()))
    assert float(err.max()) <= 2.0 * err_parent, (P, float(err.max()), err_parent)
    assert float(got[:, 3, :].abs().max()) == 0.0
    # the un-gathered form: a longer J_inv list read through win gives the same bits
    g = torch.Generator().manual_seed(P)
    win = torch.randperm(3 * P, generator=g)[:P].to(DEV)
    wide = torch.randn((3 * P, 3, 3), generator=g).to(DEV)
    wide[win] = c["J_inv"]
    assert same_bits(kernel(dfm, c, win=win, J_inv=wide), kernel(dfm, c))


def test_weights_are_the_forward_kernels(dfm):
    P = 4099
    c = make_case(dfm, P, seed=1)
    c["valid"][:] = True
    c["g_pts"].zero_()
    c["g_c2w"].fill_(1.0)
    got = kernel(dfm, c).cpu().double()
    w = dfm.query_weights(c["xc"]).cpu().double()
    want = w.sum(0)
    ceil = (P + 64) * 2.0 ** -24 * w.abs().sum(0) + 2.0 ** -149
    assert bool(((got[:, :3, :3] - want[:, None, None]).abs() <= ceil[:, None, None]).all())
    assert float(got[:, :3, 3].abs().max()) == 0.0            # g_pts = 0: no translation gradient
    assert float(got[:, 3, :].abs().max()) == 0.0


def test_invalid_points_contribute_nothing(dfm):
    c = make_case(dfm, 257, seed=2)
    c["valid"][:] = False
    got = kernel(dfm, c)
    assert got.shape == (24, 4, 4) and float(got.abs().max()) == 0.0
    e = make_case(dfm, 0)
    got = kernel(dfm, e)
    assert got.shape == (24, 4, 4) and float(got.abs().max()) == 0.0
    # a NaN at an invalid point is never read
    c = make_case(dfm, 257, seed=3)
    ref = kernel(dfm, c)
    bad = ~c["valid"]
    for k in ("g_pts", "g_c2w", "J_inv"):
        c[k][bad] = float("nan")
    assert same_bits(kernel(dfm, c), ref)


def test_reproducible(dfm):
    c = make_case(dfm, 4099, seed=4)
    a, b = kernel(dfm, c), kernel(dfm, c)
    assert same_bits(a, b)
    # more tiles than blocks (2048 tiles of 256 points): the strided walk over the tiles, still one fixed order
    big = make_case(dfm, 2048 * 256 + 257 + 3, seed=5)
    a, b = kernel(dfm, big), kernel(dfm, big)
    assert same_bits(a, b)
    want, ceil = want_and_ceiling(dfm, big)
    assert bool(((a.cpu().double() - want).abs() <= ceil).all())


def test_node_forward_is_the_identity_and_its_backward_the_kernel(dfm):
    c = make_case(dfm, 257, seed=6)
    tfs0 = dfm.tfs
    try:
        dfm.tfs = tfs0.detach().clone().requires_grad_(True)
        pts, c2w = dfm.pose_terms(c["xc"], c["c2w"], c["J_inv"], c["valid"])
        assert same_bits(pts.detach(), c["xc"]) and same_bits(c2w.detach(), c["c2w"])
        assert pts.requires_grad and c2w.requires_grad
        torch.autograd.backward([pts, c2w], [c["g_pts"], c["g_c2w"]])
        assert dfm.tfs.grad.shape == (1, 24, 4, 4) and same_bits(dfm.tfs.grad[0], kernel(dfm, c))
    finally:
        dfm.tfs = tfs0


def _step(rs, rays, target, tmask):
    dfm = rs.deformer
    tfs0 = dfm.tfs
    try:
        dfm.tfs = tfs0.detach().clone().requires_grad_(True)
        for p in rs.parameters():
            p.grad = None
        out = rs.forward_backward(rays, target, tmask)
        return out, dfm.tfs.grad.detach().clone()
    finally:
        dfm.tfs = tfs0


def test_node_equals_the_parent_route_in_shade_differentiable(frame, monkeypatch):
    """train.shade_differentiable with tfs.requires_grad (as tests/test_gpu_train.py::test_pose_gradients_vs_torch_autograd sets it
    up): the node against the old expressions patched back in.  Forward: the same bits.  tfs.grad: both routes reduce the same
    per-sample gradients (captured by hooks on the node's outputs); each is held to the fp64 reduction of those, the node under the
    ceiling and within 2 x the parent route's error."""
    from intrinsicavatar_amd.deformer import SNARFDeformer
    rs, rays = frame
    n = rays.shape[0]
    g = torch.Generator().manual_seed(5)
    target = torch.rand((n, 3), generator=g).cuda()
    tmask = (torch.rand(n, generator=g) > 0.5).float().cuda()
    seen = {}
    real = SNARFDeformer.pose_terms

    def spy(self, xc, c2w, J_inv, valid, win=None):
        pts, c2 = real(self, xc, c2w, J_inv, valid, win)
        seen.update(xc=xc, c2w=c2w, J_inv=J_inv, valid=valid)
        pts.register_hook(lambda gr: seen.__setitem__("g_pts", gr.detach().clone()))
        c2.register_hook(lambda gr: seen.__setitem__("g_c2w", gr.detach().clone()))
        return pts, c2

    monkeypatch.setattr(SNARFDeformer, "pose_terms", spy)
    out_new, grad_new = _step(rs, rays, target, tmask)
    assert out_new["n_samples"] > 300 and bool(out_new["valid"].any())

    def old(self, xc, c2w, J_inv, valid, win=None):
        pts, R = self.implicit_pose_terms(xc, J_inv, valid)
        return pts, c2w + (R - R.detach()) * valid[:, None, None].to(R.dtype)

    monkeypatch.setattr(SNARFDeformer, "pose_terms", old)
    out_old, grad_old = _step(rs, rays, target, tmask)
    for k in ("loss", "comp_rgb", "comp_normal", "opacity", "sdf", "sdf_grad", "c2w", "pts_cano", "rgbs", "alphas"):
        assert same_bits(out_new[k].detach(), out_old[k].detach()), k
    want, ceil = want_and_ceiling(rs.deformer, seen)
    err_new = (grad_new[0].cpu().double() - want).abs()
    err_old = (grad_old[0].cpu().double() - want).abs()
    print(f"shade_differentiable: node max abs error {float(err_new.max()):.3e}, parent route {float(err_old.max()):.3e}, "
          f"largest entry {float(want.abs().max()):.3e}")
    assert float(want.abs().max()) > 0
    assert bool((err_new <= ceil).all())
    assert float(err_new.max()) <= 2.0 * float(err_old.max())


def test_pbr_path_carries_the_pose_gradient(frame, monkeypatch):
    """train_phys.shade_differentiable_phys: with tfs.requires_grad the node is attached (tfs.grad is the fp64 reduction of the
    gradients that reach its two outputs); without, the dict is the one of a run that never asks (same bits)."""
    from intrinsicavatar_amd import fields, pbr, train_phys
    from intrinsicavatar_amd.deformer import SNARFDeformer
    rs, rays = frame
    dfm = rs.deformer
    mat = fields.VolumeMaterial(seed=2).to(DEV)
    env = pbr.EnvironmentLightSG(num_SGs=8, base_res=16, seed=1).to(DEV)
    g = torch.Generator().manual_seed(7)
    spp = 512
    light_u, shuffle_u = torch.rand((512, 3), generator=g).to(DEV), torch.rand((rays.shape[0], spp), generator=g).to(DEV)
    rays_o, rays_d, far, t_starts, t_ends, ray_indices, packed_info, _ = rs.sample(rays)
    jit = torch.randn((t_starts.shape[0], 3), generator=g).to(DEV)
    target = torch.rand((rays.shape[0], 3), generator=g).to(DEV)

    def run():
        return train_phys.shade_differentiable_phys(rs, mat, env, rays_o, rays_d, ray_indices, t_starts, t_ends, packed_info, spp, light_u,
                                                    shuffle_u, env_base=env.generate_image(), jitter_n=jit)

    seen = {}
    real = SNARFDeformer.pose_terms

    def spy(self, xc, c2w, J_inv, valid, win=None):
        pts, c2 = real(self, xc, c2w, J_inv, valid, win)
        seen.update(xc=xc, c2w=c2w, J_inv=J_inv, valid=valid, calls=seen.get("calls", 0) + 1)
        pts.register_hook(lambda gr: seen.__setitem__("g_pts", gr.detach().clone()))
        c2.register_hook(lambda gr: seen.__setitem__("g_c2w", gr.detach().clone()))
        return pts, c2

    monkeypatch.setattr(SNARFDeformer, "pose_terms", spy)
    base = run()
    assert "calls" not in seen                                   # tfs is a constant: the node is not even built
    tfs0 = dfm.tfs
    try:
        dfm.tfs = tfs0.detach().clone().requires_grad_(True)
        out = run()
        loss = train_phys.training_loss_phys(out, target, None, lambda_smooth=0.01)
        loss.backward()
        grad = dfm.tfs.grad
        assert grad is not None and grad.shape == (1, 24, 4, 4) and bool(torch.isfinite(grad).all())
        with torch.no_grad():                                    # grad mode off: no node either
            quiet = run()
    finally:
        dfm.tfs = tfs0
    assert seen["calls"] == 1 and out["stats"]["n_fg"] > 0
    want, ceil = want_and_ceiling(dfm, seen)
    assert float(want.abs().max()) > 0 and float(seen["g_pts"].abs().max()) > 0 and float(seen["g_c2w"].abs().max()) > 0
    assert bool(((grad[0].cpu().double() - want).abs() <= ceil).all())
    again = run()
    for k, v in base.items():
        if isinstance(v, torch.Tensor):
            assert same_bits(v.detach(), again[k].detach()), k
            assert same_bits(v.detach(), quiet[k].detach()), k
