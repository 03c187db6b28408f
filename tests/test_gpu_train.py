"""GPU: forward+backward of the training step -- every parameter gradient produced by the HIP backward
kernels (incl. the second-order path through the analytic normal) vs float64 torch autograd on the same samples.
Tolerance: 2e-3 relative to the largest gradient entry of each tensor (fp32 kernels, atomics, fast exp)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def frame():
    from intrinsicavatar_amd import build
    build.build()
    from intrinsicavatar_amd import synthetic as S
    rs, rays, export = S.build_frame("cuda:0", 48, 48, pose_seed=1, beta=0.05, num_samples_per_ray=32, grid_D=16, grid_H=64,
                                     grid_W=64, smooth_iters=3, hash_amp=3e-2)
    torch.manual_seed(1234)                    # the perturbation below defines the problem instance: keep it fixed
    with torch.no_grad():                      # make every weight matter
        for p in rs.radiance.network.parameters():
            p.add_(torch.randn_like(p) * 0.05)
        for p in rs.geometry.network.parameters():     # sphere init zeroes the hash-feature columns of W1
            p.add_(torch.randn_like(p) * 0.03)
    rs.geometry.update_step(0, 1500)           # progressive masks: 12 of 16 levels
    rs.radiance.update_step(0, 1500)
    return rs, rays


@pytest.mark.parametrize("lambda_curv", [0.0, 0.5])
def test_forward_backward_vs_torch_autograd(frame, lambda_curv):
    """lambda_curv > 0 adds the curvature regulariser (second SDF evaluation at x + 1e-4 tangent, geometry.py:173-203)."""
    from tests import torch_ref as TR
    rs, rays = frame
    n = rays.shape[0]
    g = torch.Generator().manual_seed(0)
    target = torch.rand((n, 3), generator=g).cuda()
    tmask = (torch.rand(n, generator=g) > 0.5).float().cuda()
    curv_u = torch.rand((200000, 3), generator=g).cuda() if lambda_curv > 0 else None
    for p in rs.parameters():
        p.grad = None
    out = rs.forward_backward(rays, target, tmask, curv_u=curv_u, lambda_curv=lambda_curv)
    assert out["n_samples"] > 3000 and bool(out["valid"].any())
    geo, rad, dens = rs.geometry, rs.radiance, rs.density
    D = lambda t: t.detach().cpu().double()      # noqa: E731
    l0, l2 = geo.network.layers[0], geo.network.layers[2]
    rl = rad.network.layers
    P = dict(geo_center=D(geo.center), geo_scale=D(geo.scale), geo_table=D(geo.grid_params), geo_mask=D(geo.prog.mask(1500, "cpu")),
             geo_g0=D(l0.weight_g), geo_v0=D(l0.weight_v), geo_b0=D(l0.bias), geo_g2=D(l2.weight_g), geo_v2=D(l2.weight_v),
             geo_b2=D(l2.bias), beta=D(dens.beta), rad_center=D(rad.center), rad_scale=D(rad.scale), rad_table=D(rad.grid_params),
             rad_mask=D(rad.prog.mask(1500, "cpu")), rad_sh_mask=D(rad.sh_mask[0]),
             rad_W0=D(rl[0].weight), rad_b0=D(rl[0].bias), rad_W2=D(rl[2].weight), rad_b2=D(rl[2].bias),
             rad_W4=D(rl[4].weight), rad_b4=D(rl[4].bias))
    leaves = ["geo_table", "geo_g0", "geo_v0", "geo_b0", "geo_g2", "geo_v2", "geo_b2", "beta", "rad_table", "rad_W0", "rad_b0",
              "rad_W2", "rad_b2", "rad_W4", "rad_b4"]
    for k in leaves:
        P[k].requires_grad_(True)
    rays_s = rs.deformer.transform_rays_w2s(rays.float())
    pi = rs.sample(rays)[6]
    fixed = dict(pts_cano=D(out["pts_cano"]), valid=out["valid"].cpu(), c2w=D(out["c2w"]), w2s_rot=D(rs.deformer.w2s[:3, :3]),
                 rays_d=D(rays_s[:, 3:6]), ray_indices=None, t_starts=None, t_ends=None, n_rays=n, packed_info=pi.cpu())
    # recover the sample set of the step (deterministic: sample() twice gives the same set)
    _, _, _, ts, te, ri, pi2, _ = rs.sample(rays)
    assert ts.shape[0] == out["n_samples"]
    fixed.update(ray_indices=ri.cpu(), t_starts=D(ts), t_ends=D(te), packed_info=pi2.cpu())
    if lambda_curv > 0:
        fixed["curv_u"] = D(curv_u[:ts.shape[0]])
    loss_ref, ref = TR.shade_reference(P, fixed, D(target), D(tmask), lambda_curv=lambda_curv)
    loss_ref.backward()
    assert abs(float(out["loss"]) - float(loss_ref)) < 2e-4 * max(1.0, abs(float(loss_ref)))
    # fp32 (kernels) vs fp64 (reference): a sample within rounding distance of a hash-cell face lands in the
    # neighbouring cell, where the analytic normal (piecewise constant per cell) differs -> rare outliers
    err = np.abs(out["comp_rgb"].detach().cpu().numpy() - ref["comp_rgb"].detach().numpy())
    assert (err > 2e-4).mean() < 5e-3 and err.max() < 3e-2, (float((err > 2e-4).mean()), float(err.max()))
    got = dict(geo_table=geo.grid_params.grad, geo_g0=l0.weight_g.grad, geo_v0=l0.weight_v.grad, geo_b0=l0.bias.grad,
               geo_g2=l2.weight_g.grad, geo_v2=l2.weight_v.grad, geo_b2=l2.bias.grad, beta=dens.beta.grad,
               rad_table=rad.grid_params.grad, rad_W0=rl[0].weight.grad, rad_b0=rl[0].bias.grad, rad_W2=rl[2].weight.grad,
               rad_b2=rl[2].bias.grad, rad_W4=rl[4].weight.grad, rad_b4=rl[4].bias.grad)
    worst = {}
    for k in leaves:
        a, b = got[k].detach().cpu().double(), P[k].grad
        assert a is not None and b is not None, k
        scale = float(b.abs().max())
        assert scale > 0, f"reference gradient of {k} is identically zero -- test is vacuous"
        if k.endswith("_table"):
            # sparse atomic scatter: a sample that lands in the neighbouring hash cell in fp32 vs fp64 moves its
            # whole contribution to other entries -> judge the table gradients by relative L2 error
            worst[k] = float((a - b).norm() / b.norm())
        else:
            worst[k] = float((a - b).abs().max()) / scale
    print(worst)
    bad = {k: v for k, v in worst.items() if v > (3e-2 if k.endswith('_table') else 5e-3)}
    assert not bad, worst


def test_pose_gradients_vs_torch_autograd(frame):
    """bone transforms as an optimised input (pose_correction, snarf_deformer.py:93-105): d loss / d tfs through the
    implicit-function correction of the canonical roots (ForwardDeformer.forward version 1, deformer_torch.py:57-76) and the
    blended-rotation normal push-forward, against fp64 autograd of the same formulas on the same sample set.  The second
    derivative of the hash encoding w.r.t. its input is dropped on both sides (tests/torch_ref.py:_HashEncRef)."""
    from tests import torch_ref as TR
    rs, rays = frame
    n = rays.shape[0]
    g = torch.Generator().manual_seed(5)
    target = torch.rand((n, 3), generator=g).cuda()
    tmask = (torch.rand(n, generator=g) > 0.5).float().cuda()
    dfm = rs.deformer
    tfs0 = dfm.tfs
    try:
        dfm.tfs = tfs0.detach().clone().requires_grad_(True)
        for p in rs.parameters():
            p.grad = None
        out = rs.forward_backward(rays, target, tmask)
        got = dfm.tfs.grad.detach().cpu().double()[0]
        table_grad_pose = rs.geometry.grid_params.grad.detach().clone()
        assert "J_inv" in out and out["n_samples"] > 3000
        geo, rad, dens = rs.geometry, rs.radiance, rs.density
        D = lambda t: t.detach().cpu().double()      # noqa: E731
        l0, l2 = geo.network.layers[0], geo.network.layers[2]
        rl = rad.network.layers
        P = dict(geo_center=D(geo.center), geo_scale=D(geo.scale), geo_table=D(geo.grid_params),
                 geo_mask=D(geo.prog.mask(1500, "cpu")), geo_g0=D(l0.weight_g), geo_v0=D(l0.weight_v), geo_b0=D(l0.bias),
                 geo_g2=D(l2.weight_g), geo_v2=D(l2.weight_v), geo_b2=D(l2.bias), beta=D(dens.beta), rad_center=D(rad.center),
                 rad_scale=D(rad.scale), rad_table=D(rad.grid_params), rad_mask=D(rad.prog.mask(1500, "cpu")),
                 rad_sh_mask=D(rad.sh_mask[0]), rad_W0=D(rl[0].weight), rad_b0=D(rl[0].bias), rad_W2=D(rl[2].weight),
                 rad_b2=D(rl[2].bias), rad_W4=D(rl[4].weight), rad_b4=D(rl[4].bias), tfs=D(dfm.tfs[0]))
        P["tfs"].requires_grad_(True)
        P["geo_table"].requires_grad_(True)
        rays_s = dfm.transform_rays_w2s(rays.float())
        _, _, _, ts, te, ri, pi, _ = rs.sample(rays)
        assert ts.shape[0] == out["n_samples"]
        with torch.no_grad():
            lbs_w = dfm.query_weights(out["pts_cano"].detach())
        c2w0 = out["c2w"].detach()
        fixed = dict(pts_cano=D(out["pts_cano"]), valid=out["valid"].cpu(), c2w=D(c2w0), w2s_rot=D(dfm.w2s[:3, :3]),
                     rays_d=D(rays_s[:, 3:6]), ray_indices=ri.cpu(), t_starts=D(ts), t_ends=D(te), n_rays=n,
                     packed_info=pi.cpu(), lbs_w=D(lbs_w), J_inv=D(out["J_inv"]))
        loss_ref, _ = TR.shade_reference(P, fixed, D(target), D(tmask))
        loss_ref.backward()
        want = P["tfs"].grad
        assert abs(float(out["loss"]) - float(loss_ref)) < 2e-4 * max(1.0, abs(float(loss_ref)))
        scale = float(want.abs().max())
        assert scale > 0 and bool(torch.isfinite(got).all())
        # the bottom row of each 4x4 never enters LBS of a point (x_h[3] = 1 multiplies column 3 only of rows 0..2)
        assert float(got[:, 3, :].abs().max()) == 0.0 and float(want[:, 3, :].abs().max()) == 0.0
        err = float((got - want).abs().max()) / scale
        rel = float((got - want).norm() / want.norm())
        print("pose grad: max err / max", err, "rel L2", rel, "scale", scale)
        assert err < 2e-2 and rel < 2e-2, (err, rel)
        # the parameter gradients are unaffected by the (zero-valued) correction
        tg = P["geo_table"].grad
        assert float((table_grad_pose.cpu().double() - tg).norm() / tg.norm()) < 3e-2
    finally:
        dfm.tfs = tfs0


def test_fused_mlp_backward_matches_operand_path():
    """csrc/mlp_train.hip (operands in LDS, dW in MFMA accumulators) == csrc/mlp_bwd.hip + ia_wgrad (operands through
    HBM) for the radiance head and the SDF head incl. its second-order terms; ragged n (not a multiple of 32).
    Each path against fp64 autograd, all kinds and sizes: tests/test_gpu_backward_kernels.py."""
    import ctypes as C
    from intrinsicavatar_amd import build
    build.build()
    from intrinsicavatar_amd import _lib as L, train
    g = torch.Generator().manual_seed(5)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.3).to(DEV)      # noqa: E731
    n = 100_003
    enc, xyz, feat, sh, nrm = r(n, 32), r(n, 3), r(n, 13), r(n, 16), r(n, 3)
    W1, b1, W2, b2, W3, b3 = r(64, 67), r(64), r(64, 64), r(64), r(3, 64), r(3)
    g_rgb = r(n, 3)
    segs = [(enc, 32, 1.0, 0.0), (xyz, 3, 2.0, -1.0), (feat, 13, 1.0, 0.0), (sh, 16, 1.0, 0.0), (nrm, 3, 1.0, 0.0)]
    ns, ptrs, strides, widths, muls, adds = train._segs(segs)
    z = lambda *s: torch.zeros(*s, device=DEV)      # noqa: E731
    gx_a, gx_b = torch.empty((n, 68), device=DEV), torch.empty((n, 68), device=DEV)
    X = torch.empty((n, 68), device=DEV)
    A1, A2, G1, G2 = (torch.empty((n, 64), device=DEV) for _ in range(4))
    G3 = torch.empty((n, 16), device=DEV)
    lib = L.lib()
    L.check(lib.ia_mlp_bwd(L.i32(1), L.i64(n), L.i32(ns), ptrs, strides, widths, muls, adds, L.ptr(W1), L.ptr(b1), L.ptr(W2),
                           L.ptr(b2), L.ptr(W3), L.ptr(b3), L.ptr(g_rgb), L.ptr(gx_a), L.i32(68), L.ptr(X), L.ptr(A1), L.ptr(A2),
                           L.ptr(G1), L.ptr(G2), L.ptr(G3), L.stream()))
    ref = [train.wgrad(G1, 64, X, 67), train.wgrad(G2, 64, A1, 64), train.wgrad(G3, 3, A2, 64)]
    d = [z(64, 67), z(64), z(64, 64), z(64), z(3, 64), z(3)]
    L.check(lib.ia_mlp_bwd_fused(L.i32(1), L.i64(n), L.i32(ns), ptrs, strides, widths, muls, adds, L.ptr(W1), L.ptr(b1),
                                 L.ptr(W2), L.ptr(b2), L.ptr(W3), L.ptr(b3), L.ptr(g_rgb), L.ptr(gx_b), L.i32(68),
                                 *[L.ptr(t) for t in d], L.stream()))

    def close(a, b, what):
        scale = float(b.abs().max()) + 1e-12
        assert float((a - b).abs().max()) < 2e-4 * scale, (what, float((a - b).abs().max()), scale)
    assert torch.equal(gx_a[:, :67], gx_b[:, :67])                       # same MFMA chain per point: bit-equal
    for i, (dw, db) in enumerate(ref):
        close(d[2 * i], dw, f"dW{i + 1}")
        close(d[2 * i + 1], db, f"db{i + 1}")
    # ---- SDF head
    W1s, b1s, Wo, bo = r(64, 35), r(64), r(13, 64), r(13)
    jac, g_out, q = r(n, 32, 3), r(n, 13), r(n, 3)
    ns, ptrs, strides, widths, muls, adds = train._segs([(enc, 32, 1.0, 0.0), (xyz, 3, 2.0, -1.0)])
    gE_a, gG_a, gE_b, gG_b = (torch.empty((n, 32), device=DEV) for _ in range(4))
    Hh, U = torch.empty((n, 36), device=DEV), torch.empty((n, 36), device=DEV)
    DZ, GZ, A, DGS = (torch.empty((n, 64), device=DEV) for _ in range(4))
    L.check(lib.ia_sdf_mlp_bwd(L.i64(n), L.i32(ns), ptrs, strides, widths, muls, adds, L.ptr(W1s), L.ptr(b1s), L.ptr(Wo),
                               L.ptr(bo), L.ptr(jac), L.ptr(g_out), L.ptr(q), L.ptr(gE_a), L.ptr(gG_a), L.ptr(Hh), L.ptr(U),
                               L.ptr(DZ), L.ptr(GZ), L.ptr(A), L.ptr(DGS), L.stream()))
    dW1, db1 = train.wgrad(DZ, 64, Hh, 35)
    dW1 = dW1 + train.wgrad(GZ, 64, U, 35, want_bias=False)[0]
    dWo, dbo = train.wgrad(g_out, 13, A, 64)
    dWo[0] += train.wgrad(DGS, 64, DGS, 1)[1]
    e = [z(64, 35), z(64), z(13, 64), z(13)]
    L.check(lib.ia_sdf_mlp_bwd_fused(L.i64(n), L.i32(ns), ptrs, strides, widths, muls, adds, L.ptr(W1s), L.ptr(b1s), L.ptr(Wo),
                                     L.ptr(bo), L.ptr(jac), L.ptr(g_out), L.ptr(q), L.ptr(gE_b), L.ptr(gG_b),
                                     *[L.ptr(t) for t in e], L.ptr(None), L.stream()))
    assert torch.equal(gE_a, gE_b) and torch.equal(gG_a, gG_b)
    for got, want, what in zip(e, (dW1, db1, dWo, dbo), ("dW1", "db1", "dWo", "dbo")):
        close(got, want, "sdf " + what)


def test_phys_training_step_gradients():
    """BASELINE config 4 shape (small frame): training step with the PBR branch.  Every parameter group receives a finite,
    non-zero gradient, and directional derivatives of the loss agree with central finite differences for parameters of
    each new component (environment light, material head, radiance hash table, SDF head) -- the loss is evaluated by the
    same kernels, all random inputs are explicit, so the only noise is fp32 round-off."""
    from intrinsicavatar_amd import build
    build.build()
    from intrinsicavatar_amd import synthetic as S, fields, pbr, train_phys
    rs, rays, _ = S.build_frame(DEV, 48, 48, pose_seed=0, beta=0.05, num_samples_per_ray=64, grid_D=16, grid_H=64, grid_W=64,
                                smooth_iters=5, hash_amp=1e-2)
    mat = fields.VolumeMaterial(seed=2).to(DEV)
    yy, xx = np.meshgrid(np.linspace(0, np.pi, 32), np.linspace(-np.pi, np.pi, 64), indexing="ij")
    sky = (0.6 + 0.35 * np.cos(yy)[..., None] * np.array([1.0, 0.8, 0.6]) + 0.05 * np.sin(2 * xx)[..., None]).astype(np.float32)
    env = pbr.EnvironmentLightTensor(torch.from_numpy(sky).to(DEV)); env.update_pdf()
    n = rays.shape[0]
    g = torch.Generator().manual_seed(3)
    target = torch.rand((n, 3), generator=g).to(DEV)
    spp = 512
    light_u = torch.rand((spp, 3), generator=g).to(DEV)
    shuffle_u = torch.rand((n, spp), generator=g).to(DEV)
    env_base = env.base.detach().clone().requires_grad_(True)
    params = rs.parameters() + list(mat.parameters())
    jitter_n = torch.randn((400000, 3), generator=g).to(DEV)          # material jitter pass noise (explicit)

    def run(backward):
        s = rs.sample(rays, None)
        rays_o, rays_d, far, t_starts, t_ends, ray_indices, packed_info, _ = s
        out = train_phys.shade_differentiable_phys(rs, mat, env, rays_o, rays_d, ray_indices, t_starts, t_ends, packed_info, spp,
                                                   light_u, shuffle_u, render_mode="uniform_light", env_base=env_base,
                                                   background_color=torch.zeros(3, device=DEV), jitter_n=jitter_n)
        loss = train_phys.training_loss_phys(out, target, None, lambda_eik=0.0, lambda_smooth=0.05, lambda_orient=0.05)
        if backward:
            loss.backward()
        return float(loss.detach().double()), out

    for p in params:
        p.grad = None
    l0, out = run(True)
    assert out["stats"]["n_fg"] > 1000 and out["stats"]["n_secondary"] > 100
    assert torch.isfinite(out["comp_rgb_phys"]).all()
    for k in ("albedo_smoothness_loss_map", "roughness_smoothness_loss_map", "metallic_smoothness_loss_map",
              "normals_orientation_loss_map"):
        assert torch.isfinite(out[k]).all() and float(out[k].detach().max()) > 0, k
    grads = {id(p): p.grad.clone() for p in params if p.grad is not None}
    for name, p in [("env", env_base)] + [(f"mat{i}", q) for i, q in enumerate(mat.parameters())] + \
                   [("rad_table", rs.radiance.grid_params), ("geo_table", rs.geometry.grid_params)]:
        gr = p.grad
        assert gr is not None and torch.isfinite(gr).all(), name
        if p.numel() > 1:       # (the Lipschitz bounds are inactive at init: scale = min(c / |W|_inf, 1) = 1 -> zero gradient)
            assert float(gr.abs().max()) > 0, name

    def fd(p, direction, eps):
        with torch.no_grad():
            p.add_(direction, alpha=eps)
            lp, _ = run(False)
            p.add_(direction, alpha=-2 * eps)
            lm, _ = run(False)
            p.add_(direction, alpha=eps)
        return (lp - lm) / (2 * eps)

    mp = list(mat.parameters())
    checks = [("env base", env_base, env_base.grad, 2e-2), ("material W3", mp[2], mp[2].grad, 2e-2),
              ("material W1", mp[0], mp[0].grad, 2e-2)]
    for name, p, gr, eps in checks:
        d = gr / gr.norm().clamp_min(1e-20)                          # steepest-ascent direction: largest signal
        with torch.no_grad():
            want = fd(p, d, eps * float(p.detach().abs().mean() + 1e-3))
        got = float((gr * d).sum())
        assert abs(got - want) < 0.08 * abs(want) + 1e-6, (name, got, want)


def test_gradients_are_additive_over_ray_shards(frame):
    """the multi-GPU contract: with a sum-reduced loss, the gradient of a ray batch equals the SUM of the gradients of its
    shards (what all-reduce(sum) over ray-batch-sharded ranks computes) -- for every parameter incl. both hash tables."""
    from intrinsicavatar_amd import train
    rs, rays = frame
    n = rays.shape[0]
    g = torch.Generator().manual_seed(11)
    target = torch.rand((n, 3), generator=g).cuda()

    def grads(sel):
        for p in rs.parameters():
            p.grad = None
        r = rays[sel].contiguous()
        rays_o, rays_d, far, ts, te, ri, pi, _ = rs.sample(r, None)
        out = train.shade_differentiable(rs, rays_o, rays_d, ri, ts, te, pi)
        loss = (out["comp_rgb"] - target[sel]).abs().sum() + 0.1 * ((torch.linalg.norm(out["sdf_grad"], dim=-1) - 1.0) ** 2
                                                                      * out["valid"].float()).sum()
        loss.backward()
        return [p.grad.detach().double().clone() if p.grad is not None else None for p in rs.parameters()]

    idx = torch.arange(n, device="cuda")
    full = grads(idx)
    parts = [grads(idx[: n // 3]), grads(idx[n // 3: n // 3 + 777]), grads(idx[n // 3 + 777:])]
    for k, gf in enumerate(full):
        if gf is None:
            continue
        gs = sum(p[k] for p in parts)
        scale = float(gf.abs().max()) + 1e-30
        assert float((gf - gs).abs().max()) < 2e-5 * scale + 1e-9, (k, float((gf - gs).abs().max()), scale)


def test_pose_parameters_receive_gradients_through_smpl_kinematics():
    """caller side of the deformer (snarf_deformer.py:87-126): body_pose -> SMPL forward kinematics (smpl.py, pinned
    against the reference's lbs()) -> tfs -> fast-SNARF precompute + search -> render -> loss; the pose gradient of
    shade_differentiable reaches the axis-angle parameters.  The kinematics reproduce the synthetic rig of the bench."""
    from intrinsicavatar_amd import build
    build.build()
    from intrinsicavatar_amd import synthetic as S, smpl
    rs, rays, _ = S.build_frame(DEV, 64, 64, pose_seed=0, beta=0.02, num_samples_per_ray=64, grid_D=16, grid_H=64, grid_W=64,
                                smooth_iters=3, hash_amp=2e-3)
    dfm = rs.deformer
    J = torch.from_numpy(S.JOINTS).to(DEV)
    eye = torch.eye(24, device=DEV)
    body = smpl.SMPLKinematics(J, torch.zeros((24, 3, 1), device=DEV), torch.zeros((207, 72), device=DEV), eye,
                               S.PARENTS.tolist(), eye)
    pose = torch.from_numpy(S.make_pose(0)).float().to(DEV)[None].requires_grad_(True)
    transl = torch.tensor([[0.0, 0.15, 5.0]], device=DEV)
    out = body.forward(torch.zeros((1, 1), device=DEV), pose[:, 3:], pose[:, :3], transl)
    tfs, w2s = smpl.deformer_transforms(out["A"], torch.eye(4, device=DEV).expand(1, 24, 4, 4))
    assert torch.allclose(tfs.detach(), dfm.tfs, atol=2e-5) and torch.allclose(w2s[0].detach(), dfm.w2s, atol=2e-5)
    tfs0, w2s0 = dfm.tfs, dfm.w2s
    try:
        dfm.prepare(tfs, w2s[0].detach())
        assert dfm.tfs.requires_grad
        n = rays.shape[0]
        g = torch.Generator().manual_seed(2)
        target = torch.rand((n, 3), generator=g).cuda()
        for p in rs.parameters():
            p.grad = None
        res = rs.forward_backward(rays, target, None)
        assert res["n_samples"] > 1000
        gp = pose.grad
        assert gp is not None and bool(torch.isfinite(gp).all())
        per_joint = gp.reshape(24, 3).norm(dim=1)
        assert float(per_joint.max()) > 0
        # the root rotation cancels in tfs = inverse(A_root) A (the deformer works in the SMPL-root frame): its gradient
        # through tfs is zero up to rounding, while limb joints carry most of it
        assert float(per_joint[0]) < 1e-3 * float(per_joint.max())
        assert int((per_joint > 1e-3 * per_joint.max()).sum()) >= 10
    finally:
        dfm.prepare(tfs0, w2s0)


def test_training_step_with_rays_that_miss_everything(frame):
    """a ray shard can be empty of samples (rays that miss the occupancy grid; multi-GPU ray-batch sharding makes that a
    real case): every kernel on the path sees n = 0, the loss reduces to the background terms and backward still runs."""
    rs, rays = frame
    away = rays[:4096].clone()
    away[:, 3:6] = -away[:, 3:6]                     # look away from the subject
    g = torch.Generator().manual_seed(0)
    target = torch.rand((away.shape[0], 3), generator=g).cuda()
    tmask = torch.zeros(away.shape[0], device=DEV)
    for p in rs.parameters():
        p.grad = None
    out = rs.forward_backward(away, target, tmask)
    assert out["n_samples"] == 0
    assert torch.isfinite(out["loss"]) and float(out["opacity"].abs().max()) == 0.0
    for p in rs.parameters():
        assert p.grad is None or bool(torch.isfinite(p.grad).all())
    # inference form too
    res = rs.forward(away)
    assert float(res["opacity"].abs().max()) == 0.0 and res["stats"]["n_samples"] == 0


def test_phys_training_step_vs_torch_autograd():
    """BASELINE config 4: the training step WITH the PBR branch (material head, volume-interaction gathers, uniform_light
    estimator at spp 512, composite, L1 on the physically based image) against float64 torch autograd of the same
    computation (tests/torch_ref.py shade_reference_phys) on the sample set / secondary rays the GPU found: loss, the
    physically based image and the gradients of every parameter group incl. the material head, its Lipschitz bounds, both
    hash tables and the environment texels."""
    from intrinsicavatar_amd import build
    build.build()
    from intrinsicavatar_amd import synthetic as S, fields, pbr, train_phys
    from tests import torch_ref as TR
    rs, rays, _ = S.build_frame(DEV, 40, 40, pose_seed=0, beta=0.05, num_samples_per_ray=64, grid_D=16, grid_H=64, grid_W=64,
                                smooth_iters=5, hash_amp=1e-2)
    mat = fields.VolumeMaterial(seed=2).to(DEV)
    with torch.no_grad():
        for c in mat.network.lipshitz_bound_per_layer:
            c.mul_(0.35)                                              # make the Lipschitz clamp ACTIVE (else its gradient is 0)
    yy, xx = np.meshgrid(np.linspace(0, np.pi, 32), np.linspace(-np.pi, np.pi, 64), indexing="ij")
    sky = (0.6 + 0.35 * np.cos(yy)[..., None] * np.array([1.0, 0.8, 0.6]) + 0.05 * np.sin(2 * xx)[..., None]).astype(np.float32)
    env = pbr.EnvironmentLightTensor(torch.from_numpy(sky).to(DEV)); env.update_pdf()
    n = rays.shape[0]
    g = torch.Generator().manual_seed(3)
    target = torch.rand((n, 3), generator=g).to(DEV)
    tmask = (torch.rand(n, generator=g) > 0.5).float().to(DEV)
    spp = 512
    light_u = torch.rand((spp, 3), generator=g).to(DEV)
    shuffle_u = torch.rand((n, spp), generator=g).to(DEV)
    env_base = env.base.detach().clone().requires_grad_(True)
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    params = rs.parameters() + list(mat.parameters())
    for p in params:
        p.grad = None
    rays_o, rays_d, far, ts, te, ri, pi, _ = rs.sample(rays, None)
    out = train_phys.shade_differentiable_phys(rs, mat, env, rays_o, rays_d, ri, ts, te, pi, spp, light_u, shuffle_u,
                                               render_mode="uniform_light", env_base=env_base, background_color=bg)
    loss = train_phys.training_loss_phys(out, target, tmask)
    loss.backward()
    vi = out["volume_interaction"]
    assert vi.F > 5000 and out["stats"]["n_secondary"] > 1000
    geo, rad, dens = rs.geometry, rs.radiance, rs.density
    D = lambda t: t.detach().cpu().double()      # noqa: E731
    l0, l2 = geo.network.layers[0], geo.network.layers[2]
    rl = rad.network.layers
    P = dict(geo_center=D(geo.center), geo_scale=D(geo.scale), geo_table=D(geo.grid_params), geo_mask=D(geo.prog.mask(geo.global_step, "cpu")),
             geo_g0=D(l0.weight_g), geo_v0=D(l0.weight_v), geo_b0=D(l0.bias), geo_g2=D(l2.weight_g), geo_v2=D(l2.weight_v),
             geo_b2=D(l2.bias), beta=D(dens.beta), rad_center=D(rad.center), rad_scale=D(rad.scale), rad_table=D(rad.grid_params),
             rad_mask=D(rad.prog.mask(rad.global_step, "cpu")), rad_sh_mask=D(rad.sh_mask[0]),
             rad_W0=D(rl[0].weight), rad_b0=D(rl[0].bias), rad_W2=D(rl[2].weight), rad_b2=D(rl[2].bias),
             rad_W4=D(rl[4].weight), rad_b4=D(rl[4].bias), env_base=D(env_base))
    for i in range(3):
        P[f"mat_W{i}"], P[f"mat_b{i}"] = D(mat.network.weights_per_layer[i]), D(mat.network.biases_per_layer[i])
        P[f"mat_c{i}"] = D(mat.network.lipshitz_bound_per_layer[i])
    leaves = ["geo_table", "geo_v0", "geo_b0", "geo_v2", "beta", "rad_table", "rad_W0", "rad_W4", "env_base"] + \
             [f"mat_{k}{i}" for i in range(3) for k in "Wbc"]
    for k in leaves:
        P[k].requires_grad_(True)
    # the deformer's winners (recomputed: deterministic) for the reference's fixed sample set
    from intrinsicavatar_amd import render
    pts = render.ray_points(rays_o, rays_d, ri, ts, te)
    d = rs.deformer.deform(pts, geo, with_grad=False, with_feature=False, want_fwd=True)
    sel = d["sel"].long().clamp(min=0)
    c2w = d["fwd_J"].reshape(-1, 3, 3)[d["cand_src"].long()[sel]]
    fixed = dict(pts_cano=D(d["pts_cano"]), valid=d["valid"].cpu(), c2w=D(c2w), w2s_rot=D(rs.deformer.w2s[:3, :3]), rays_d=D(rays_d),
                 ray_indices=ri.cpu(), t_starts=D(ts), t_ends=D(te), n_rays=n, packed_info=pi.cpu(),
                 fg_src=vi.fg_src.long().cpu(), fg_ray=vi.fg_ray.long().cpu(), fg_counts=vi.fg_counts.cpu(),
                 has_samples=(vi.resampled_packed_info[:, 1] > 0).cpu(), has_bg=(vi.bg_counts > 0).cpu(),
                 out_dirs=D(out["out_dirs"]), sec_tr=D(out["secondary_tr"][:, 0]), inv_pdf=D(out["inv_pdf"][:, 0]),
                 env_R=D(rs.deformer.w2s[:3, :3]))
    loss_ref, ref = TR.shade_reference_phys(P, fixed, D(target), D(tmask), D(bg))
    loss_ref.backward()
    assert abs(float(loss) - float(loss_ref)) < 5e-4 * max(1.0, abs(float(loss_ref))), (float(loss), float(loss_ref))
    err = np.abs(out["comp_rgb_phys"].detach().cpu().numpy() - ref["comp_rgb_phys"].detach().numpy())
    assert (err > 1e-3).mean() < 1e-2 and err.max() < 0.1, (float((err > 1e-3).mean()), float(err.max()))
    got = dict(geo_table=geo.grid_params.grad, geo_v0=l0.weight_v.grad, geo_b0=l0.bias.grad, geo_v2=l2.weight_v.grad, beta=dens.beta.grad,
               rad_table=rad.grid_params.grad, rad_W0=rl[0].weight.grad, rad_W4=rl[4].weight.grad, env_base=env_base.grad)
    for i in range(3):
        got[f"mat_W{i}"], got[f"mat_b{i}"] = mat.network.weights_per_layer[i].grad, mat.network.biases_per_layer[i].grad
        got[f"mat_c{i}"] = mat.network.lipshitz_bound_per_layer[i].grad
    worst = {}
    for k in leaves:
        a, b = got[k].detach().cpu().double().reshape(-1), P[k].grad.reshape(-1)
        assert float(b.abs().max()) > 0, f"reference gradient of {k} is identically zero -- test is vacuous"
        worst[k] = float((a - b).norm() / b.norm()) if (k.endswith("_table") or k == "env_base") else float((a - b).abs().max() / b.abs().max())
    print(worst)
    bad = {k: v for k, v in worst.items() if v > (5e-2 if (k.endswith("_table") or k == "env_base") else 1e-2)}
    assert not bad, worst


def test_pipelined_half_frames_match_the_sequential_chunk_loop():
    """train_phys.forward_backward_phys_pipelined (EXPERIMENTAL, off by default: IA_FRAME_PIPELINE): two ray chunks of one frame on two host
    threads / HIP streams against the same chunks processed one after the other with gradient accumulation -- the same sample counts and the
    same accumulated parameter gradients (each chunk's backward is what the sequential loop computes for it; the two-term sums meet in
    AccumulateGrad)."""
    from intrinsicavatar_amd import build
    build.build()
    from intrinsicavatar_amd import synthetic as S, fields, pbr, train_phys
    rs, rays, _ = S.build_frame(DEV, 48, 48, pose_seed=0, beta=0.05, num_samples_per_ray=64, grid_D=16, grid_H=64, grid_W=64,
                                smooth_iters=5, hash_amp=1e-2)
    mat = fields.VolumeMaterial(seed=2).to(DEV)
    yy, xx = np.meshgrid(np.linspace(0, np.pi, 32), np.linspace(-np.pi, np.pi, 64), indexing="ij")
    sky = (0.6 + 0.35 * np.cos(yy)[..., None] * np.array([1.0, 0.8, 0.6]) + 0.05 * np.sin(2 * xx)[..., None]).astype(np.float32)
    env = pbr.EnvironmentLightTensor(torch.from_numpy(sky).to(DEV)); env.update_pdf()
    n = rays.shape[0]
    g = torch.Generator().manual_seed(5)
    target = torch.rand((n, 3), generator=g).to(DEV)
    tmask = (torch.rand(n, generator=g) > 0.5).float().to(DEV)
    spp = 16
    h = n // 2
    # explicit random numbers per chunk, so that both schedules draw the same ones: per-point light directions (training form of `light`)
    lu = [torch.rand((h * spp + 4096, 3), generator=g).to(DEV), torch.rand(((n - h) * spp + 4096, 3), generator=g).to(DEV)]
    views = [(rays[:h].contiguous(), target[:h].contiguous(), tmask[:h].contiguous(), h / n),
             (rays[h:].contiguous(), target[h:].contiguous(), tmask[h:].contiguous(), (n - h) / n)]
    params = rs.parameters() + [p for p in mat.parameters() if p.requires_grad] + [env.base]
    kw = dict(render_mode="light", background_color=torch.ones(3, device=DEV), global_illumination=True, light_sampling="per_point")

    def zero():
        for p in params:
            p.grad = None

    zero()
    stats = []
    for (r, t, m, frac), u in zip(views, lu):
        o = rs.forward_backward_phys(r, t, mat, env, spp, u, None, target_mask=m, loss_scale=frac, **kw)
        stats.append(int(o["stats"]["n_fg"]))
    torch.cuda.synchronize()
    seq = [p.grad.detach().double().clone() for p in params]
    assert all(torch.isfinite(t_).all() for t_ in seq) and sum(float(t_.abs().sum()) for t_ in seq) > 0

    # the pipelined entry point draws its light directions on the device (light_u None): patch the per-chunk uniforms in through the views
    orig = rs.forward_backward_phys
    it = iter(lu)
    lock = __import__("threading").Lock()
    by_rays = {views[0][0].data_ptr(): lu[0], views[1][0].data_ptr(): lu[1]}

    def with_u(r, t, material, emitter, spp_, light_u, shuffle_u, **k):
        return orig(r, t, material, emitter, spp_, by_rays[r.data_ptr()], shuffle_u, **k)
    zero()
    rs.forward_backward_phys = with_u
    try:
        tot = train_phys.forward_backward_phys_pipelined(rs, views, mat, env, spp, n_workers=2, **kw)
    finally:
        del rs.forward_backward_phys
    torch.cuda.synchronize()
    assert tot["n_fg"] == sum(stats)
    for p, a in zip(params, seq):
        b = p.grad.detach().double()
        scale = float(a.abs().max()) + 1e-30
        # table gradients are float-atomic sums inside each chunk's backward (order varies run to run): 2e-5 of the largest entry
        assert float((a - b).abs().max()) <= 2e-5 * scale + 1e-12, (tuple(p.shape), float((a - b).abs().max()), scale)
