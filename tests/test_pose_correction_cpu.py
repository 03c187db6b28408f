"""Pose correction without a GPU: the module against a restatement of the reference's forward / update_step
(models/pose/pose_correction.py), the step-order arithmetic of fit.Trainer, FitConfig.check_scope with and without a module, the
optimiser group, and the C ABI of the fused pose-term backward."""
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = 5


def ref_forward(weights, enabled, idx):
    """models/pose/pose_correction.py:25-47 on a dict of the four weight tensors"""
    if enabled:
        betas = weights["shape_correction"][torch.zeros(1).long()]
        orient = weights["global_orient_correction"][idx]
        transl = weights["transl_correction"][idx]
        pose = weights["pose_correction"][idx]
    else:
        betas = torch.zeros_like(weights["shape_correction"])
        orient = torch.zeros_like(weights["global_orient_correction"][:1])
        transl = torch.zeros_like(weights["transl_correction"][:1])
        pose = torch.zeros_like(weights["pose_correction"][:1])
    return dict(betas_correction=betas, global_orient_correction=orient, transl_correction=transl, pose_correction=pose)


def ref_enabled_after(config_enable, start, steps):
    """the switch after update_step(epoch, s) for s in steps (:49-54)"""
    on = False
    for s in steps:
        if config_enable and s > start:
            on = True
    return on


def module(**kw):
    from intrinsicavatar_amd.pose_correction import PoseCorrection
    return PoseCorrection(F, **kw)


def test_parameters_names_shapes_and_zero_init():
    m = module(enable_pose_correction=True)
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {"pose_correction.weight": (F, 69), "shape_correction.weight": (1, 10),
                                                          "global_orient_correction.weight": (F, 3), "transl_correction.weight": (F, 3)}
    assert all(float(v.abs().max()) == 0.0 for v in sd.values())
    assert all(p.requires_grad for p in m.parameters()) and len(list(m.parameters())) == 4
    assert m.enable_pose_correction is False


@pytest.mark.parametrize("enabled", [False, True])
def test_forward_matches_the_reference(enabled):
    m = module(enable_pose_correction=True, pose_correction_start_step=0)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    m.enable_pose_correction = enabled
    weights = {k[:-len(".weight")]: v for k, v in m.state_dict().items()}
    for idx in (torch.tensor([3]), torch.tensor([0, 4, 4])):
        got, want = m(idx), ref_forward(weights, enabled, idx)
        assert sorted(got) == sorted(want) == ["betas_correction", "global_orient_correction", "pose_correction", "transl_correction"]
        for k in want:
            assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
        # disabled: zeros of one row whatever idx is; the shape row never depends on idx
        assert got["betas_correction"].shape == (1, 10)
        if not enabled:
            assert got["pose_correction"].shape == (1, 69) and all(float(v.abs().max()) == 0.0 for v in got.values())
        else:
            assert got["pose_correction"].shape == (len(idx), 69) and torch.equal(got["betas_correction"], weights["shape_correction"])


def test_update_step_compares_strictly_and_never_switches_off():
    for start in (0, 1, 4000):
        m = module(enable_pose_correction=True, pose_correction_start_step=start)
        for s in range(start + 3):
            m.update_step(0, s)
            assert m.enable_pose_correction == (s > start) == ref_enabled_after(True, start, range(s + 1)), (start, s)
        m.update_step(0, 0)
        assert m.enable_pose_correction                      # nothing turns it off
    off = module(enable_pose_correction=False, pose_correction_start_step=0)
    off.update_step(0, 10 ** 6)
    assert not off.enable_pose_correction and not ref_enabled_after(False, 0, [10 ** 6])


def first_corrected_step(start):
    """fit.Trainer.step's order: the frame is posed with the switch as the previous step left it, then update_step(global_step)"""
    m = module(enable_pose_correction=True, pose_correction_start_step=start)
    for step in range(start + 10):
        posed_with_corrections = m.enable_pose_correction
        m.update_step(0, step)
        if posed_with_corrections:
            return step
    return None


def test_the_first_corrected_step_is_start_plus_two():
    from intrinsicavatar_amd import fit
    for start in (0, 1, 7, 4000):
        assert first_corrected_step(start) == start + 2
    assert fit.FitConfig().pose_correction_start_step == 4000 and fit.FitConfig().pose_correction_wd == 1e-5
    assert "S + 2" in fit.__doc__
    # the schedule itself knows nothing of the module: its phases are the same with the flag set
    cfg = fit.FitConfig(enable_pose_correction=True)
    assert fit.Schedule(cfg).at(4001) == fit.Schedule(fit.FitConfig()).at(4001)


def test_check_scope_with_and_without_a_module():
    from intrinsicavatar_amd import fit
    fit.FitConfig().check_scope()
    fit.FitConfig().check_scope(module())
    cfg = fit.FitConfig(enable_pose_correction=True)
    with pytest.raises(NotImplementedError, match=r"fit\.Trainer: out of scope -- .*enable_pose_correction"):
        cfg.check_scope()
    cfg.check_scope(module(enable_pose_correction=True))
    # what stays refused stays refused, module or not
    for kw in (dict(optimize_betas=True), dict(reinit_optimizer_steps=[100]), dict(world_size=2)):
        with pytest.raises(NotImplementedError, match="out of scope"):
            fit.FitConfig(enable_pose_correction=True, **kw).check_scope(module(enable_pose_correction=True))
    c = fit.FitConfig(enable_pose_correction=True)
    c.system["reinit_shape_every_n_steps"] = 10
    with pytest.raises(NotImplementedError, match="reinit_shape_every_n_steps"):
        c.check_scope(module(enable_pose_correction=True))


def test_param_groups_gain_one_group_only_with_a_module():
    from intrinsicavatar_amd import optim

    class Mod(torch.nn.Module):
        def __init__(self, n):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(n))

    class RS:
        geometry, radiance, density = Mod(2), Mod(3), Mod(1)
    RS.radiance.grid_params = RS.radiance.p
    RS.radiance.q = torch.nn.Parameter(torch.zeros(4))
    base = optim.reference_param_groups(RS)
    m = module(enable_pose_correction=True)
    with_pc = optim.reference_param_groups(RS, pose_correction=m)
    assert [g["name"] for g in with_pc] == [g["name"] for g in base] + ["pose_correction"]
    for a, b in zip(base, with_pc):
        assert a.keys() == b.keys() and all(a[k] is b[k] or a[k] == b[k] for k in a if k != "params")
        assert all(x is y for x, y in zip(a["params"], b["params"]))
    pc = with_pc[-1]
    assert pc["lr"] == 1e-4 and pc["weight_decay"] == 1e-5 and len(pc["params"]) == 4
    assert optim.reference_param_groups(RS, pose_correction=m, pose_correction_wd=0.5)[-1]["weight_decay"] == 0.5


def test_header_declares_the_pose_term_backward():
    import ctypes as C
    from intrinsicavatar_amd import _lib, build
    protos = _lib.header_prototypes()
    assert "ia_pose_terms_bwd" in protos and "ia_pose_terms_bwd_tmp_size" in protos
    restype, args = protos["ia_pose_terms_bwd"]
    assert restype is C.c_int and len(args) == 17 and args[0] is C.c_int64 and args[-1] is C.c_void_p
    assert [i for i, a in enumerate(args) if a is C.c_int] == [9, 10, 11]                 # D, H, W as ia_forward_skinning takes them
    assert "ia_pose_terms_bwd_tmp_size" in _lib.header_host_only() and "ia_pose_terms_bwd" not in _lib.header_host_only()
    assert "pose_terms.hip" in build.SOURCES and "-ffp-contract=off" in build.SOURCES["pose_terms.hip"]
    assert os.path.exists(os.path.join(ROOT, "intrinsicavatar_amd", "csrc", "pose_terms.hip"))
    # the work area: one layout function, measured and carved by the same code; a function of P alone, capped by the block count
    lib = C.CDLL(build.build())
    q = lib.ia_pose_terms_bwd_tmp_size
    q.restype, q.argtypes = C.c_int64, [C.c_int64]
    block = 24 * 12 * 8
    assert q(0) == 0 and q(1) == block and q(256) == block and q(257) == 2 * block
    assert q(2048 * 256) == 2048 * block == q(10 ** 9)
