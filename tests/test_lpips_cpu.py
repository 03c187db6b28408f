"""CPU: LPIPS without a GPU -- the entry points of csrc/lpips.hip are declared and exported, the Python interfaces exist with their stated
defaults and refuse host tensors, check_state_dicts names what is wrong, and the restatement tests/lpips_ref.py is what it claims."""
import ctypes
import inspect

import pytest
import torch

from tests import lpips_ref as R
from tests.test_abi_cpu import so_path      # noqa: F401   (the module-scoped fixture that builds the library)

ENTRY_POINTS = ("ia_lpips_pixels_per_partial", "ia_lpips_input", "ia_lpips_conv3x3", "ia_lpips_maxpool2", "ia_lpips_layer_dist",
                "ia_lpips_finish")


def test_entry_points_are_declared_exported_and_none_is_a_byte_query(so_path):      # noqa: F811
    from intrinsicavatar_amd import _lib, build
    protos = _lib.header_prototypes()
    lib = ctypes.CDLL(so_path)
    ours = sorted(n for n in protos if n.startswith("ia_lpips_"))
    assert ours == sorted(ENTRY_POINTS)
    for name in ours:
        assert hasattr(lib, name), name
        assert not name.endswith("_bytes"), name
    host_only = _lib.header_host_only()
    assert {n for n in ours if n in host_only} == {"ia_lpips_pixels_per_partial"}          # every launching entry point takes a stream
    assert "lpips.hip" in build.SOURCES
    assert lib.ia_lpips_pixels_per_partial() >= 1


def test_check_state_dicts_names_the_missing_key_and_the_wrong_shape():
    from intrinsicavatar_amd import metrics as M
    vgg, lin = R.random_weights(1)
    M.LPIPSNet.check_state_dicts(vgg, lin)
    for key in ("features.0.weight", "features.28.bias", "features.14.weight"):
        bad = dict(vgg)
        del bad[key]
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            M.LPIPSNet.check_state_dicts(bad, lin)
    bad = dict(lin)
    del bad["lin3.model.1.weight"]
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight"):
        M.LPIPSNet.check_state_dicts(vgg, bad)
    bad = dict(vgg)
    bad["features.17.weight"] = torch.zeros((512, 512, 3, 3))
    with pytest.raises(ValueError, match=r"features\.17\.weight.*\(512, 512, 3, 3\)"):
        M.LPIPSNet.check_state_dicts(bad, lin)
    bad = dict(lin)
    bad["lin1.model.1.weight"] = torch.zeros((1, 64, 1, 1))
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight.*\(1, 64, 1, 1\)"):
        M.LPIPSNet.check_state_dicts(vgg, bad)


def test_keys_and_signatures():
    from intrinsicavatar_amd import metrics as M, system
    assert system.METRIC_KEYS == ("rf_psnr", "rf_ssim", "normal_error", "pbr_psnr", "pbr_ssim", "albedo_psnr", "albedo_ssim")
    assert system.LPIPS_KEYS == ("rf_lpips", "pbr_lpips", "albedo_lpips")
    for fn in (system.evaluate_frame, system.evaluate_sequence):
        p = inspect.signature(fn).parameters["lpips"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, fn
    assert list(inspect.signature(M.LPIPS.forward).parameters) == ["self", "inputs", "targets", "loss_fn_vgg", "valid_mask"]
    p = inspect.signature(M.LPIPSNet.forward).parameters
    assert list(p) == ["self", "in0", "in1", "normalize", "rect"] and p["normalize"].default is False and p["rect"].default is None
    assert list(inspect.signature(M.LPIPSNet.from_state_dicts).parameters) == ["vgg16_state", "lin_state", "device"]
    assert list(inspect.signature(M.LPIPSNet.from_files).parameters) == ["vgg_path", "lin_path", "device"]
    assert 3 in M._STATUS and "16" in M._STATUS[3]
    assert "LPIPS is not provided" not in M.__doc__
    assert M.VGG_CONVS == R.CONVS and M.VGG_TAPS == R.TAPS and M.VGG_POOL_BEFORE == R.POOL_BEFORE


def test_there_is_no_host_route():
    from intrinsicavatar_amd import _lib, metrics as M
    vgg, lin = R.random_weights(1)
    with pytest.raises(_lib.IaError):
        M.LPIPSNet.from_state_dicts(vgg, lin, "cpu")
    net = M.LPIPSNet([], [])
    with pytest.raises(_lib.IaError):
        net(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16))
    with pytest.raises(_lib.IaError):
        M.LPIPS()(torch.rand(16, 16, 3), torch.rand(16, 16, 3), net)


def test_the_restatement_is_zero_on_identical_images_and_equals_the_literal_formula():
    vgg, lin = R.random_weights(2)
    g = torch.Generator().manual_seed(3)
    a, b = torch.rand((1, 3, 16, 16), generator=g), torch.rand((1, 3, 16, 16), generator=g)
    assert float(R.lpips_ref(a, a, vgg, lin, normalize=True, dtype=torch.float64)) == 0.0
    got = R.lpips_ref(a, b, vgg, lin, normalize=True, dtype=torch.float64)
    assert tuple(got.shape) == (1, 1, 1, 1) and got.dtype == torch.float64 and float(got) > 0.0
    # literally, layer by layer with loops over the pixels
    dt = torch.float64
    shift, scale = torch.tensor(R.SHIFT, dtype=torch.float32).to(dt), torch.tensor(R.SCALE, dtype=torch.float32).to(dt)
    F = torch.nn.functional

    def taps(x):
        x = ((2 * x.to(dt) - 1) - shift.view(1, 3, 1, 1)) / scale.view(1, 3, 1, 1)
        out = []
        for idx in range(29):
            if idx in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28):
                x = F.conv2d(x, vgg[f"features.{idx}.weight"].to(dt), vgg[f"features.{idx}.bias"].to(dt), padding=1).clamp_min(0)
                if idx in (2, 7, 14, 21, 28):
                    out.append(x[0])
            elif idx in (4, 9, 16, 23):
                x = F.max_pool2d(x, kernel_size=2, stride=2)
        return out
    want = 0.0
    for i, (fa, fb) in enumerate(zip(taps(a), taps(b))):
        C, h, w = fa.shape
        assert (C, h, w) == (R.TAP_CHANNELS[i], 16 >> i, 16 >> i)
        lw = lin[f"lin{i}.model.1.weight"].to(dt).reshape(C)
        s = 0.0
        for y in range(h):
            for x in range(w):
                u = fa[:, y, x] / (fa[:, y, x].pow(2).sum().sqrt() + 1e-10)
                v = fb[:, y, x] / (fb[:, y, x].pow(2).sum().sqrt() + 1e-10)
                s += float((lw * (u - v) ** 2).sum())
        want += s / (h * w)
    assert abs(float(got) - want) <= 1e-12 * want
    # the float32 evaluation sits at float32 distance
    assert abs(float(R.lpips_ref(a, b, vgg, lin, normalize=True, dtype=torch.float32)) - want) <= 1e-4 * want
