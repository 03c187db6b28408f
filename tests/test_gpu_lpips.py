"""GPU (MI355X): LPIPS (csrc/lpips.hip, metrics.LPIPSNet / metrics.LPIPS, system.evaluate_frame(lpips=...)) piece by piece -- one
convolution layer against fp64 under the forward-error bound of its fmaf chain, the rectangle read from the device against a physical
crop, the max-pool, the whole distance against tests/lpips_ref.py in float64, the criterion, and the frame evaluation.

Weights are random (tests/lpips_ref.random_weights: N(0, 2 / (9 Cin)) convolutions, small biases, lin >= 0), images uniform in [0,1].
The observed figures are printed; with IA_LPIPS_PARITY_OBSERVE=<file> they are also collected there (profiles/lpips_parity.json is that
file from a run on the MI355X)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import forward_golden as FG
from tests import lpips_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_OBSERVE = os.environ.get("IA_LPIPS_PARITY_OBSERVE")
F = torch.nn.functional


def _observe(section, key, value):
    print("lpips parity", section, key, value)
    if _OBSERVE:
        old = json.load(open(_OBSERVE)) if os.path.exists(_OBSERVE) else {}
        old.setdefault(section, {})[key] = value
        os.makedirs(os.path.dirname(os.path.abspath(_OBSERVE)), exist_ok=True)
        json.dump(old, open(_OBSERVE, "w"), indent=1, sort_keys=True)


def B(t):
    return t.detach().as_subclass(torch.Tensor).cpu().numpy().tobytes()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.fixture(scope="module")
def M():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from intrinsicavatar_amd import build, metrics
    build.build()
    return metrics


@pytest.fixture(scope="module")
def weights():
    return R.random_weights(0)


@pytest.fixture(scope="module")
def net(M, weights):
    return M.LPIPSNet.from_state_dicts(*weights, DEV)


def _layer(M, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = 0.05 * torch.randn(cout, generator=g)
    return w, b, M.pack_conv3x3(w, b, DEV)


def _pad4(x):
    """[N,H,W,C] -> C rounded up to 4 with zeros (the first layer takes the input stage's 4 channels)"""
    pad = -x.shape[-1] % 4
    return torch.cat([x, torch.zeros(x.shape[:-1] + (pad,), dtype=x.dtype)], dim=-1) if pad else x


CONV_SHAPES = ((2, 37, 45, 3, 64), (1, 19, 23, 64, 128), (1, 9, 11, 256, 256), (1, 5, 4, 512, 512), (1, 2, 3, 512, 512), (1, 1, 1, 512, 512))


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_convolution_layer_against_fp64(M, shape):
    """|y - y64| <= (K + 2) 2^-24 S with K = 9 Cin and S = conv3x3(|x|, |w|) + |b| in fp64: the forward-error bound of a length-K fmaf
    chain plus the bias add; ReLU is 1-Lipschitz.  Observed on the MI355X: profiles/lpips_parity.json `conv_max_err_over_S`."""
    N, H, W, cin, cout = shape
    w, b, (wpk, bias) = _layer(M, cin, cout, 10 + cin + H)
    g = torch.Generator().manual_seed(H * W)
    x = torch.randn((N, cin, H, W), generator=g)
    y = M.lpips_conv3x3(_pad4(nhwc(x)).to(DEV), wpk, bias).cpu().permute(0, 3, 1, 2).double()
    assert tuple(y.shape) == (N, cout, H, W)
    y64 = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1))
    S = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=1)
    err = (y - y64).abs()
    _observe("conv_max_err_over_S", "x".join(map(str, shape)), float((err / S).max()))
    assert bool((err <= (9 * cin + 2) * 2.0 ** -24 * S).all()), float((err / S).max())
    assert float(y64.max()) > 0.0 and float(y.min()) >= 0.0


@pytest.mark.parametrize("shape", ((2, 37, 45, 3, 64), (1, 19, 23, 64, 128), (1, 2, 3, 512, 512), (1, 1, 1, 512, 512)),
                         ids=lambda s: "x".join(map(str, s)))
def test_all_ones_counts_the_taps_inside(M, shape):
    N, H, W, cin, cout = shape
    wpk, bias = M.pack_conv3x3(torch.ones((cout, cin, 3, 3)), torch.zeros(cout), DEV)
    y = M.lpips_conv3x3(_pad4(torch.ones((N, H, W, cin))).to(DEV), wpk, bias).cpu()
    rows = torch.minimum(torch.arange(H) + 1, torch.tensor(H - 1)) - torch.clamp(torch.arange(H) - 1, min=0) + 1
    cols = torch.minimum(torch.arange(W) + 1, torch.tensor(W - 1)) - torch.clamp(torch.arange(W) - 1, min=0) + 1
    want = (rows[:, None] * cols[None, :] * cin).float()
    if H >= 3 and W >= 3:
        assert sorted(set((want / cin).flatten().tolist())) == [4.0, 6.0, 9.0]
    assert torch.equal(y, want[None, :, :, None].expand(N, H, W, cout))


RECTS = ((5, 3, 21, 17), (25, 23, 21, 17))              # odd x, y, w, h; the second touches the right and the bottom border of 40 x 46


@pytest.mark.parametrize("rect", RECTS, ids=str)
def test_rectangle_from_the_device_is_the_physical_crop(M, rect):
    H, W = 40, 46
    x0, y0, w, h = rect
    assert x0 + w <= W and y0 + h <= H
    drect = torch.tensor(rect, dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(7)
    # the input stage + the first layer on images
    img = torch.rand((2, H, W, 3), generator=g).to(DEV)
    crop = img[:, y0:y0 + h, x0:x0 + w].contiguous()
    _, _, (wpk0, b0) = _layer(M, 3, 64, 1)
    for normalize in (False, True):
        s_full, s_crop = M.lpips_input(img, normalize, drect), M.lpips_input(crop, normalize)
        assert B(s_full[:, :h, :w]) == B(s_crop)
        assert B(M.lpips_conv3x3(s_full, wpk0, b0, drect)[:, :h, :w]) == B(M.lpips_conv3x3(s_crop, wpk0, b0))
    # a 64 -> 128 layer read at the rectangle's corner of a larger feature map: the surroundings must not leak into the halo
    _, _, (wpk, b) = _layer(M, 64, 128, 2)
    feat = torch.randn((2, H, W, 64), generator=g).to(DEV)
    want = M.lpips_conv3x3(feat[:, y0:y0 + h, x0:x0 + w].contiguous(), wpk, b)
    assert B(M.lpips_conv3x3(feat, wpk, b, drect, 0, True)[:, :h, :w]) == B(want)
    # ... and at level 1 the extent is (h >> 1, w >> 1) at the origin, for the pool and for the layer behind it
    pooled = M.lpips_maxpool2(feat, drect, 0)
    assert tuple(pooled.shape) == (2, H // 2, W // 2, 64)
    want_pool = M.lpips_maxpool2(feat[:, :h, :w].contiguous())
    assert tuple(want_pool.shape) == (2, h // 2, w // 2, 64) and B(pooled[:, :h // 2, :w // 2]) == B(want_pool)
    assert B(M.lpips_conv3x3(pooled, wpk, b, drect, 1)[:, :h // 2, :w // 2]) == B(M.lpips_conv3x3(want_pool, wpk, b))


@pytest.mark.parametrize("hw", ((37, 45), (5, 3)), ids=str)
def test_max_pool_is_torchs(M, hw):
    H, W = hw
    x = torch.randn((2, 64, H, W), generator=torch.Generator().manual_seed(H))
    got = M.lpips_maxpool2(nhwc(x).to(DEV)).cpu().permute(0, 3, 1, 2)
    assert torch.equal(got, F.max_pool2d(x, 2))


SIZES = ((16, 16), (37, 45), (64, 48))


def _pairs(hw, n=8):
    g = torch.Generator().manual_seed(100 + hw[0])
    return torch.rand((n, 3) + hw, generator=g), torch.rand((n, 3) + hw, generator=g)


@pytest.fixture(scope="module")
def references(weights):
    """per size: (ref64, ref32) of the eight pairs, float64 / float32 on the CPU, computed once"""
    out = {}
    for hw in SIZES:
        a, b = _pairs(hw)
        out[hw] = (R.lpips_ref(a, b, *weights, normalize=True, dtype=torch.float64),
                   R.lpips_ref(a, b, *weights, normalize=True, dtype=torch.float32).double())
    return out


@pytest.mark.parametrize("hw", SIZES, ids=str)
def test_end_to_end_against_the_float64_restatement(net, references, hw):
    """e_ours = max |ours - ref64| <= 4 e_fp32 = 4 max |ref32 - ref64| over the same eight pairs: two fp32 evaluations with different
    summation orders sit at the same order of distance from fp64, a wrong tap / channel / pooling phase shows at 1e-3 of the value.
    Observed on the MI355X: profiles/lpips_parity.json `end_to_end`."""
    a, b = _pairs(hw)
    ref64, ref32 = references[hw]
    ours = net(a.to(DEV), b.to(DEV), normalize=True)
    assert tuple(ours.shape) == (8, 1, 1, 1) and ours.is_cuda and ours.dtype == torch.float32
    ours = ours.cpu().double()
    e_ours, e_fp32 = float((ours - ref64).abs().max()), float((ref32 - ref64).abs().max())
    _observe("end_to_end", f"{hw[0]}x{hw[1]}", dict(e_ours=e_ours, e_fp32=e_fp32, smallest_value=float(ref64.min())))
    assert e_ours <= 4.0 * e_fp32, (e_ours, e_fp32)


def test_end_to_end_invariants(M, net, weights):
    a, b = (t.to(DEV) for t in _pairs((37, 45), 3))
    d = net(a, b, normalize=True)
    assert torch.equal(net(a, a).as_subclass(torch.Tensor), torch.zeros((3, 1, 1, 1), device=DEV))          # identical images: exactly 0
    assert B(net(b, a, normalize=True)) == B(d)                                                              # symmetric
    assert B(net(a[2:3], b[2:3], normalize=True)) == B(d[2:3])                                               # slot 2 of N = 3 is N = 1
    assert B(net(2 * a - 1, 2 * b - 1)) == B(d)                                                              # normalize is 2x - 1
    assert B(net(a, b, normalize=True)) == B(d)                                                              # run to run
    assert float(d.min()) > 0.0 and all(np.isfinite(v) for v in d.reshape(-1).tolist())
    # a fifth tap that is zero everywhere (its last bias far below every pre-activation): 0 / (0 + 1e-10), not 0 / 0
    vgg = dict(weights[0])
    vgg["features.28.bias"] = torch.full((512,), -1e4)
    dead = M.LPIPSNet.from_state_dicts(vgg, weights[1], DEV)
    f = dead.features(nhwc(a), True)
    assert float(f[4].abs().max()) == 0.0 and float(f[3].abs().max()) > 0.0
    v = dead(a, b, normalize=True).cpu()
    assert bool(torch.isfinite(v).all()) and float(v.min()) > 0.0


def _masked_pair(w_rect):
    """two 40 x 46 images and a ragged mask whose bounding rectangle is (5, 3, w_rect, 17)"""
    g = torch.Generator().manual_seed(11)
    a, b = torch.rand((40, 46, 3), generator=g), torch.rand((40, 46, 3), generator=g)
    mask = torch.zeros((40, 46), dtype=torch.bool)
    mask[4:19, 6:5 + w_rect - 1] = torch.rand((15, w_rect - 2), generator=g) > 0.4
    mask[3, 9] = mask[19, 11] = mask[8, 5] = mask[10, 5 + w_rect - 1] = True
    return a.to(DEV), b.to(DEV), mask.to(DEV)


def test_criterion_crops_on_the_device(M, net):
    a, b, mask = _masked_pair(21)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        v = M.LPIPS()(a, b, net, mask)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert v.is_cuda and v.dim() == 0 and v.dtype == torch.float32
    x, y, w, h = M.mask_rect(mask).tolist()
    assert (x, y, w, h) == (5, 3, 21, 17)
    crop = lambda t: t[y:y + h, x:x + w][None].permute(0, 3, 1, 2)      # noqa: E731
    want = net(crop(a), crop(b), normalize=True)
    assert B(v) == B(want) and float(v) > 0.0
    assert B(M.LPIPS()(a, b, net)) == B(net(a[None].permute(0, 3, 1, 2), b[None].permute(0, 3, 1, 2), normalize=True))      # no mask
    # a rectangle 15 wide leaves nothing at the fifth tap; so does an empty mask
    a, b, mask = _masked_pair(15)
    assert M.mask_rect(mask).tolist() == [5, 3, 15, 17]
    v = M.LPIPS()(a, b, net, mask)
    assert bool(torch.isnan(v.as_subclass(torch.Tensor)))
    with pytest.raises(ValueError, match="16 pixels"):
        float(v)
    with pytest.raises(ValueError, match="16 pixels"):
        M.to_host(dict(rf_lpips=v))
    with pytest.raises(ValueError):
        float(M.LPIPS()(a, b, net, torch.zeros_like(mask)))


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_evaluate_frame_adds_the_three_values_and_changes_nothing_else(M, net):
    from intrinsicavatar_amd import system
    G = FG.load()
    base = "light_16_nogi"
    rs, mat, env, rays = FG.gpu_scene(G, base)
    rnd = FG.explicit_randoms(G, base)
    light_u, shuffle_u = T(rnd["light_u"]), T(rnd["shuffle_u"])
    kw = dict(background_color=T(G["background_color"]), global_illumination=False, render_mode="light")
    H = W = 28
    n = rays.shape[0]
    assert n == H * W
    # a test batch after preprocess_data: targets derived from a first pass, masks = the body's joined with a box so that both
    # rectangles have sides of at least 16
    first = rs.forward_(rays, mat, env, 16, light_u, shuffle_u, **kw)
    g = torch.Generator().manual_seed(5)
    noise = lambda *s: torch.rand(s, generator=g).to(DEV)      # noqa: E731

    def box(y0, y1, x0, x1):
        m = torch.zeros((H, W), dtype=torch.bool, device=DEV)
        m[y0:y1, x0:x1] = True
        return m.reshape(-1)
    hit = first["opacity"][:, 0] > 0.5
    batch = dict(rays=rays, rgb=(first["comp_rgb_phys_full"] + 0.05 * (noise(n, 3) - 0.5)).clamp(0, 1),
                 alpha=(hit | box(5, 22, 4, 21)).float() * 0.9 + 0.05, valid_mask=(first["opacity"][:, 0] > 0.1) | box(3, 24, 5, 24),
                 albedo=(first["comp_albedo_full"] * 1.3 + 0.02 * noise(n, 3)).clamp(0, 1), normal=first["comp_normal"] + 0.1,
                 w2c=torch.eye(4, device=DEV)[None], hdri=T(G["hdri"]))
    gm, vm = batch["alpha"] > 0.5, batch["valid_mask"]
    for m in (gm, vm):
        assert min(M.mask_rect(m.reshape(H, W)).tolist()[2:]) >= 16
    plain, _ = system.evaluate_frame(rs, dict(batch), mat, env, 16, light_u, shuffle_u, img_wh=(W, H), stage="test", **kw)
    assert sorted(plain) == sorted(system.METRIC_KEYS)
    calls = []
    inner = system.model_forward

    def counted(*a, **k):
        torch.cuda.set_sync_debug_mode("default")
        try:
            calls.append(1)
            return inner(*a, **k)
        finally:
            torch.cuda.set_sync_debug_mode("error")
    system.model_forward = counted
    torch.cuda.set_sync_debug_mode("error")
    try:
        metrics, res = system.evaluate_frame(rs, dict(batch), mat, env, 16, light_u, shuffle_u, img_wh=(W, H), stage="test", lpips=net, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        system.model_forward = inner
    assert len(calls) == 2
    assert sorted(metrics) == sorted(system.METRIC_KEYS + system.LPIPS_KEYS)
    for k in system.METRIC_KEYS:
        assert B(metrics[k]) == B(plain[k]), k
    img = lambda t: t.reshape(H, W, 3)      # noqa: E731
    crit = M.LPIPS()
    hand = dict(rf_lpips=crit(img(res["comp_rgb_full"]), img(batch["rgb"]), net, valid_mask=vm.reshape(H, W)),
                pbr_lpips=crit(img(res["comp_rgb_phys_full"]), img(batch["rgb"]), net, valid_mask=vm.reshape(H, W)),
                albedo_lpips=crit(img(res["aligned_albedo"]), img(batch["albedo"]), net, valid_mask=gm.reshape(H, W)))
    for k, v in hand.items():
        assert metrics[k].is_cuda and metrics[k].dim() == 0 and B(metrics[k]) == B(v), (k, float(metrics[k]), float(v))
        assert float(v) > 0.0
    host = M.to_host(metrics)
    assert sorted(host) == sorted(metrics) and all(np.isfinite(v) for v in host.values())
    mean = system.mean_metrics([metrics, metrics])
    assert list(mean) == list(metrics) and all(abs(mean[k] - host[k]) <= 1e-12 * abs(host[k]) for k in host)
    print("evaluate_frame with lpips", host)
