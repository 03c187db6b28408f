"""CPU: fit.Schedule against the reference's BaseSystem.C (tests/golden/golden_schedule.json, made by tests/golden/make_golden_fit.py
from systems/base.py at run time), fit.FitConfig against configs/config.yaml as recorded there, and the switches of the shipped
schedule at the steps where they flip."""
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(HERE, "golden", "golden_schedule.json")))


def test_C_equals_the_reference(golden):
    from intrinsicavatar_amd.fit import Schedule
    rows = golden["schedule"]
    assert len(rows) >= 150
    kinds = set()
    for r in rows:
        v = r["value"]
        got = Schedule.C(v, r["global_step"], r["epoch"])
        assert got == r["result"] and type(got) is type(r["result"]), r
        if isinstance(v, list):
            kinds.add((len(v), type(v[-1]).__name__))
    assert kinds == {(3, "int"), (3, "float"), (4, "int"), (4, "float")}


def test_C_rejects_what_the_reference_rejects():
    from intrinsicavatar_amd.fit import Schedule
    with pytest.raises(TypeError):
        Schedule.C("1.0", 0, 0)
    with pytest.raises(AssertionError):
        Schedule.C([1.0, 2.0], 0, 0)


def test_fit_config_defaults_are_the_shipped_config(golden):
    from intrinsicavatar_amd.fit import FitConfig
    cfg, want = FitConfig(), golden["fit_config"]
    for section in ("model", "loss", "trainer", "system", "optimizer"):
        got = getattr(cfg, section)
        assert got == want[section], (section, {k: (got.get(k), want[section].get(k)) for k in set(got) | set(want[section])
                                                if got.get(k) != want[section].get(k)})
        for k, v in want[section].items():
            assert type(got[k]) is type(v), (section, k)
    cfg.check_scope()


def test_switches_of_the_shipped_schedule():
    from intrinsicavatar_amd.fit import Schedule
    at = Schedule().at
    assert not at(9999).enable_phys and at(10000).enable_phys
    assert not at(1000).importance_sample and at(1001).importance_sample
    assert at(12499).with_curvature and not at(12500).with_curvature
    assert at(12499).lam["lambda_curvature"] == 1.5 and at(12500).lam["lambda_curvature"] == 0.0
    assert at(12499).lam["lambda_lipshitz_bound"] == 0 and at(12500).lam["lambda_lipshitz_bound"] == 1e-5
    assert at(0).grid_update and at(20).grid_update and not at(19).grid_update
    assert [s for s in range(25001) if at(s).reinit_grid] == [8000]
    assert at(0).jitter_materials and at(24999).jitter_materials
    lam = at(0).lam
    assert set(lam) == {k for k in Schedule().config.loss if k.startswith("lambda_")} and "sparsity_scale" not in lam


@pytest.mark.parametrize("change", [
    dict(enable_pose_correction=True), dict(optimize_betas=True), dict(reinit_optimizer_steps=[5000]), dict(world_size=2),
    dict(system=dict(reinit_shape_every_n_steps=2000)), dict(system=dict(pbr_loss_only=True)), dict(loss=dict(lambda_distortion=0.01)),
    dict(loss=dict(lambda_distortion=[0.0, 0.1, 100])), dict(loss=dict(lambda_albedo=1.0)), dict(model=dict(learned_background=True))])
def test_out_of_scope_options_raise(change):
    from intrinsicavatar_amd.fit import FitConfig
    cfg = FitConfig()
    for k, v in change.items():
        if isinstance(v, dict):
            getattr(cfg, k).update(v)
        else:
            setattr(cfg, k, v)
    with pytest.raises(NotImplementedError) as e:
        cfg.check_scope()
    assert "out of scope" in str(e.value)


def test_train_loss_entry_points_are_declared_and_not_size_queries():
    """ia_train_loss_partials counts doubles: it is not one of the *_bytes work-area queries the recorded size table covers"""
    from intrinsicavatar_amd import _lib, build, train_loss
    protos = _lib.header_prototypes()
    assert {"ia_train_loss_partials", "ia_train_loss", "ia_train_loss_bwd"} <= set(protos)
    assert "train_loss.hip" in build.SOURCES and "-ffp-contract=off" in build.SOURCES["train_loss.hip"]
    assert len(protos["ia_train_loss"][1]) == 25 and len(protos["ia_train_loss_bwd"][1]) == 30
    assert len(train_loss.TERMS) == 15 and train_loss.TERMS[10] == "curvature"
    hdr = open(os.path.join(ROOT, "include", "ia_amd.h")).read()
    assert "#define IA_TRAIN_LOSS_TERMS 16" in hdr and "#define IA_TRAIN_LOSS_STATS 18" in hdr
