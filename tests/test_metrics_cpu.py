"""CPU: frame evaluation without a GPU -- the fixture tests/golden/golden_eval.npz (tests/golden/make_golden_eval.py) is consistent with
itself, the package's metrics refuse host tensors, the new interfaces exist with their stated defaults, the library exports the kernels."""
import ctypes
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

from tests.test_abi_cpu import so_path      # noqa: F401   (the module-scoped fixture that builds the library)

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def E():
    return np.load(os.path.join(HERE, "golden", "golden_eval.npz"))


def case(E, name):
    return {k.split("/", 1)[1]: E[k] for k in E.files if k.startswith(name + "/")}


def test_reference_float32_results_agree_with_the_float64_evaluation(E):
    """float32 summation bound: relative 1e-5 on the means (5e-5 dB on PSNR follows: d(dB) = 4.34 d(mean) / mean)."""
    names = [str(n) for n in E["cases"]]
    assert len(names) == 4
    for name in names:
        c = case(E, name)
        assert abs(float(c["ref_psnr"]) - float(c["f64_psnr"])) <= 5e-5, name
        assert abs(float(c["ref_albedo_psnr"]) - float(c["f64_albedo_psnr"])) <= 5e-5, name
        np.testing.assert_allclose(c["ref_ratio"].astype(np.float64), c["f64_ratio"], rtol=1e-5, atol=0, err_msg=name)
        assert abs(float(c["ref_normal_error"]) - float(c["f64_normal_error"])) <= 1e-5 * float(c["f64_normal_error"]), name
        assert int(c["f64_normal_count"]) == int(c["gt_mask"].sum()) > 0
        assert c["ref_psnr"].dtype == np.float32 and c["ref_ratio"].dtype == np.float32 and c["ref_normal_error"].dtype == np.float32
        # the aligned albedo of the reference: zero outside the mask, clamped inside
        assert float(np.abs(c["ref_aligned"][~c["gt_mask"]]).max(initial=0.0)) == 0.0
        assert 0.0 <= float(c["ref_aligned"].min()) and float(c["ref_aligned"].max()) <= 1.0


def test_fixture_shapes_masks_and_rectangles(E):
    sizes = {"blob_96x80": (96, 80), "blob_61x47": (61, 47), "full_40x40": (40, 40)}
    for name, (H, W) in sizes.items():
        c = case(E, name)
        assert (int(c["H"]), int(c["W"])) == (H, W)
        x, y, w, h = (int(v) for v in c["rect_valid"])
        if name.startswith("blob"):
            assert x > 0 and y > 0 and x + w < W and y + h < H            # touches no image edge
            assert (x + w / 2, y + h / 2) != (W / 2, H / 2)                # off-centre
        else:
            assert (x, y, w, h) == (0, 0, W, H)
        m = c["valid_mask"].reshape(H, W)
        assert m[y:y + h, x:x + w].any(0).all() and m[y:y + h, x:x + w].any(1).all() and int(m.sum()) == int(m[y:y + h, x:x + w].sum())
    assert not any(k.startswith("nomask_") and k.endswith("/valid_mask") for k in E.files)       # the case with valid_mask = None


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_eval", os.path.join(HERE, "golden", "make_golden_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_ssim_restatement_reproduces_the_closed_form_anchors(E):
    gen = _generator()
    same = E["anchor_identical_image"]
    assert gen.ssim_restatement(same, same) == 1.0 and float(E["anchor_identical_ssim"]) == 1.0
    a, b = (np.float32(v) for v in E["anchor_constant_ab"])
    C1 = (0.01 * 2.0) ** 2
    closed = (2.0 * float(a) * float(b) + C1) / (float(a) ** 2 + float(b) ** 2 + C1)            # the float32 pixel values, widened
    got = gen.ssim_restatement(np.full((20, 22, 3), a, np.float32), np.full((20, 22, 3), b, np.float32))
    assert abs(got - closed) <= 1e-12 and abs(float(E["anchor_constant_ssim"]) - closed) <= 1e-12
    assert abs(float(E["anchor_constant_closed_form"]) - closed) == 0.0
    # the stored values are the restatement's
    c = case(E, "full_40x40")
    img = lambda t: t.reshape(40, 40, 3)      # noqa: E731
    assert abs(gen.ssim_restatement(img(c["pred_rgb"]), img(c["rgb"])) - float(c["f64_rf_ssim"])) <= 1e-15


def test_metrics_raise_on_cpu_tensors():
    from intrinsicavatar_amd import _lib, metrics as M
    a, b = torch.rand(12, 3), torch.rand(12, 3)
    m = torch.ones(12, dtype=torch.bool)
    for call in (lambda: M.PSNR()(a, b), lambda: M.PSNR()(a, b, valid_mask=m), lambda: M.NormalError()(a, b, m),
                 lambda: M.SSIM()(torch.rand(9, 9, 3), torch.rand(9, 9, 3)), lambda: M.compute_albedo_rescale_factor(a, b, m),
                 lambda: M.align_albedo(a, b, m, ratio=torch.ones(3)), lambda: M.transform_normals(a), lambda: M.mask_rect(torch.ones(4, 4, dtype=torch.bool))):
        with pytest.raises((_lib.IaError, NotImplementedError)):
            call()


def test_new_interfaces_exist_with_the_stated_defaults():
    from intrinsicavatar_amd import metrics as M, render, system
    for fn in (render.RenderStep.relight, render.RenderStep.forward_):
        p = inspect.signature(fn).parameters
        assert p["albedo_only"].default is False and p["albedo_align_ratio"].default is None, fn
    assert "albedo_align_ratio" not in inspect.signature(render.RenderStep.forward_train_).parameters       # eval only
    p = inspect.signature(system.evaluate_frame).parameters
    assert list(p)[:7] == ["rs", "batch", "material", "emitter", "spp", "light_u", "shuffle_u"] and p["shuffle_u"].default is None
    assert p["img_wh"].kind is inspect.Parameter.KEYWORD_ONLY and p["img_wh"].default is inspect.Parameter.empty
    assert p["stage"].kind is inspect.Parameter.KEYWORD_ONLY and p["stage"].default == "test"
    assert list(inspect.signature(M.PSNR.forward).parameters) == ["self", "inputs", "targets", "valid_mask", "reduction"]
    assert list(inspect.signature(M.NormalError.forward).parameters) == ["self", "inputs", "targets", "valid_mask", "reduction"]
    assert list(inspect.signature(M.SSIM.forward).parameters) == ["self", "inputs", "targets", "valid_mask"]
    assert list(inspect.signature(M.compute_albedo_rescale_factor).parameters) == ["gt_albedo", "pred_albedo", "gt_mask"]
    assert inspect.signature(M.align_albedo).parameters["ratio"].default is None
    assert inspect.signature(M.transform_normals).parameters["w2c"].default is None
    assert system.METRIC_KEYS == ("rf_psnr", "rf_ssim", "normal_error", "pbr_psnr", "pbr_ssim", "albedo_psnr", "albedo_ssim")


def test_library_exports_the_metric_kernels(so_path):      # noqa: F811
    lib = ctypes.CDLL(so_path)
    for name in ("ia_metric_sq_err", "ia_metric_albedo_sums", "ia_metric_albedo_apply", "ia_metric_transform_normals", "ia_metric_normal_error",
                 "ia_metric_mask_rect", "ia_metric_ssim", "ia_metric_tmp_bytes", "ia_metric_ssim_tmp_bytes"):
        assert hasattr(lib, name), name
    lib.ia_metric_tmp_bytes.restype = ctypes.c_int64
    lib.ia_metric_ssim_tmp_bytes.restype = ctypes.c_int64
    assert lib.ia_metric_tmp_bytes() >= 1024 * 7 * 8
    assert lib.ia_metric_ssim_tmp_bytes(540, 540, 3) == 3 * 17 * 17 * 8
