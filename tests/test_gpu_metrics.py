"""GPU (MI355X): the metric kernels (csrc/metrics.hip through intrinsicavatar_amd/metrics.py) against tests/golden/golden_eval.npz -- the
reference's own PSNR / NormalError / compute_albedo_rescale_factor / transform_normals / aligned albedo, a float64 evaluation of the same
formulas, numpy's bounding rectangles and the float64 restatement of scikit-image 0.18.1's SSIM (tests/golden/make_golden_eval.py).

Bars (derived, none taken from the code under test):
  sums            1e-10 relative to the float64 evaluation (n <= 3e5 bounded terms in fp64: n 2^-53 ~ 3e-11); counts, rectangles identical
  PSNR, ratio     float32 results within 1 ulp of the float64 value rounded to float32, and within the float32 summation bound of the
                  reference's own float32 value (5e-5 dB; 1e-5 relative)
  SSIM            1e-9 absolute (window variances err by ~1e-16 against C2 = 3.6e-3); exactly 1.0 on identical images
  normal error    2e-3 degrees on the mean: two float32 unit vectors 2 ulp apart move the cosine by <= 4e-7, at >= 1 degree (the fixture's
                  condition) that is <= 1.3e-3 degrees per pixel
  transform       2 ulp, the ulp taken at the vector's largest component: the three products of a component have the vector's magnitude
                  and may cancel (the fixture's background normal has an exactly zero x: the rotated x is ~1e-9), so a component's OWN ulp is
                  a bound no summation order meets; the vector-scale ulp is the premise of the normal-error bound above
  aligned albedo  identical where the float32 ratio is the reference's; else |d ratio| x pred (one ulp of the ratio x pred when the ratios
                  are an ulp apart) + the product's own rounding (1 ulp)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().as_subclass(torch.Tensor).cpu().numpy()


@pytest.fixture(scope="module")
def E():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from intrinsicavatar_amd import build
    build.build()
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_eval.npz"))


def case(E, name):
    return {k.split("/", 1)[1]: E[k] for k in E.files if k.startswith(name + "/")}


def names(E):
    return [str(n) for n in E["cases"]]


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32)))


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def test_reductions_against_the_float64_evaluation(E):
    from intrinsicavatar_amd import metrics as M
    for name in names(E):
        c = case(E, name)
        H, W = int(c["H"]), int(c["W"])
        vm = T(c["valid_mask"]) if "valid_mask" in c else None
        gm = T(c["gt_mask"])
        sums, psnr = M.squared_error(T(c["pred_rgb"]), T(c["rgb"]), vm)
        s = N(sums)
        print(name, "sq_err", s[0], float(c["f64_sq_err"]), "psnr", float(psnr), float(c["f64_psnr"]), float(c["ref_psnr"]))
        assert s[1] == float(c["f64_sq_count"])
        assert rel(s[0], c["f64_sq_err"]) <= 1e-10
        p = N(psnr)
        assert p.dtype == np.float32 and p.shape == ()
        want = np.float32(c["f64_psnr"])
        assert abs(float(p) - float(want)) <= float(ulp32(want)) and abs(float(p) - float(c["ref_psnr"])) <= 5e-5
        # the class with the reference's call signature returns the same bits
        assert np.array_equal(N(M.PSNR()(T(c["pred_rgb"]), T(c["rgb"]), valid_mask=vm)), p)
        sums, ratio = M.albedo_sums(T(c["albedo"]), T(c["pred_albedo"]), gm)
        s, r = N(sums), N(ratio)
        print(name, "albedo sums", s.tolist(), "ratio", r.tolist(), c["ref_ratio"].tolist())
        assert s.shape == (3, 2) and r.shape == (3,) and r.dtype == np.float32
        assert float(np.max(np.abs(s - c["f64_albedo_sums"]) / np.abs(c["f64_albedo_sums"]))) <= 1e-10
        want = c["f64_ratio"].astype(np.float32)
        assert bool((np.abs(r.astype(np.float64) - want.astype(np.float64)) <= ulp32(want)).all())
        assert bool((np.abs(r.astype(np.float64) - c["ref_ratio"]) <= 1e-5 * np.abs(c["ref_ratio"])).all())
        assert np.array_equal(N(M.compute_albedo_rescale_factor(T(c["albedo"]), T(c["pred_albedo"]), gm)), r)
        # sum of the mask, rectangles
        ne = M.normal_error(T(c["pred_normal"]), T(c["normal"]), gm, w2c=T(c["w2c"]), transform=True, normalize=True)
        assert N(ne["sums"])[1] == float(c["f64_normal_count"])
        assert np.array_equal(N(M.mask_rect(gm.reshape(H, W))), c["rect_gt"])
        if vm is not None:
            assert np.array_equal(N(M.mask_rect(vm.reshape(H, W))), c["rect_valid"])
        assert N(M.mask_rect(gm.reshape(H, W))).dtype == np.int32
    assert np.array_equal(N(M.mask_rect(torch.zeros((9, 13), dtype=torch.bool, device=DEV))), np.zeros(4, np.int32))
    one = torch.zeros((9, 13), dtype=torch.bool, device=DEV)
    one[8, 12] = True
    assert N(M.mask_rect(one)).tolist() == [12, 8, 1, 1]


def test_ssim_against_the_float64_restatement(E):
    from intrinsicavatar_amd import metrics as M
    for name in names(E):
        c = case(E, name)
        H, W = int(c["H"]), int(c["W"])
        img = lambda a: T(a).reshape(H, W, 3)      # noqa: E731
        un = M.SSIM()(img(c["pred_rgb"]), img(c["rgb"]))
        assert N(un).dtype == np.float64 and N(un).shape == ()
        print(name, "ssim unmasked", float(un), float(c["f64_rf_ssim_unmasked"]))
        assert abs(float(un) - float(c["f64_rf_ssim_unmasked"])) <= 1e-9
        pairs = [("gt_mask", "rect_gt", c["ref_aligned"], c["albedo"], "f64_albedo_ssim")]
        if "valid_mask" in c:
            pairs.append(("valid_mask", "rect_valid", c["pred_rgb"], c["rgb"], "f64_rf_ssim"))
        for mk, rk, a, b, want in pairs:
            got = M.SSIM()(img(a), img(b), valid_mask=T(c[mk]).reshape(H, W))
            print(name, want, float(got), float(c[want]))
            assert abs(float(got) - float(c[want])) <= 1e-9
            # the masked value IS the unmasked value of the pre-cropped images
            x, y, w, h = (int(v) for v in c[rk])
            crop = lambda t: t[y:y + h, x:x + w].contiguous()      # noqa: E731
            pre = M.SSIM()(crop(img(a)), crop(img(b)))
            assert N(pre).tobytes() == N(got).tobytes()
    same = T(E["anchor_identical_image"])
    assert float(M.SSIM()(same, same)) == 1.0
    big = T(case(E, "blob_96x80")["rgb"]).reshape(96, 80, 3)
    assert float(M.SSIM()(big, big)) == 1.0
    a, b = (float(v) for v in E["anchor_constant_ab"])
    ca, cb = torch.full((20, 22, 3), a, device=DEV), torch.full((20, 22, 3), b, device=DEV)
    assert abs(float(M.SSIM()(ca, cb)) - float(E["anchor_constant_closed_form"])) <= 1e-9


def test_ssim_rectangle_smaller_than_the_window_raises_when_the_value_is_read():
    from intrinsicavatar_amd import metrics as M
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand((40, 40, 3), generator=g).to(DEV), torch.rand((40, 40, 3), generator=g).to(DEV)
    m = torch.zeros((40, 40), dtype=torch.bool, device=DEV)
    m[10:30, 5:11] = True                                       # 6 wide, 20 tall
    v = M.SSIM()(a, b, valid_mask=m)                            # nothing is read back here
    assert v.is_cuda
    with pytest.raises(ValueError):
        v.item()
    with pytest.raises(ValueError):
        M.to_host({"rf_ssim": M.SSIM()(a, b, valid_mask=m)})
    with pytest.raises(ValueError):
        M.SSIM()(a, b, valid_mask=torch.zeros((40, 40), dtype=torch.bool, device=DEV)).item()          # empty mask: rectangle (0,0,0,0)
    with pytest.raises(ValueError):
        M.PSNR()(a, b, valid_mask=torch.zeros((40, 40), dtype=torch.bool, device=DEV)).item()
    m[10:30, 5:12] = True                                       # 7 wide: the smallest rectangle that has a window
    assert np.isfinite(M.SSIM()(a, b, valid_mask=m).item())


def test_normal_error_transform_and_aligned_albedo_against_the_reference(E):
    from intrinsicavatar_amd import metrics as M
    for name in names(E):
        c = case(E, name)
        gm = T(c["gt_mask"])
        cam = M.transform_normals(T(c["pred_normal"]), T(c["w2c"]))
        scale = ulp32(np.abs(c["ref_normal_cam"]).max(-1, keepdims=True))
        d = np.abs(N(cam).astype(np.float64) - c["ref_normal_cam"]) / scale
        print(name, "transform_normals: max difference in ulp of the vector's largest component", float(d.max()))
        assert float(d.max()) <= 2.0
        flip = M.transform_normals(T(c["pred_normal"]))
        assert np.array_equal(N(flip), c["pred_normal"] * np.array([1.0, -1.0, -1.0], np.float32))
        # the reference's call: NormalError(F.normalize(camera-space prediction), F.normalize(target), alpha > 0.5)
        fused = M.normal_error(T(c["pred_normal"]), T(c["normal"]), gm, w2c=T(c["w2c"]), transform=True, normalize=True, want_map=True,
                               want_camera=True)
        by_hand = M.NormalError()(torch.nn.functional.normalize(cam, dim=-1), torch.nn.functional.normalize(T(c["normal"]), dim=-1), gm)
        print(name, "normal error", float(fused["mean"]), float(by_hand), float(c["ref_normal_error"]), float(c["f64_normal_error"]))
        assert N(fused["mean"]).dtype == np.float32
        assert abs(float(fused["mean"]) - float(c["ref_normal_error"])) <= 2e-3
        assert abs(float(by_hand) - float(c["ref_normal_error"])) <= 2e-3
        assert np.array_equal(N(fused["camera"]), N(cam))
        emap = M.NormalError()(torch.nn.functional.normalize(cam, dim=-1), torch.nn.functional.normalize(T(c["normal"]), dim=-1), gm, reduction="none")
        assert float(np.abs(N(emap) - c["ref_normal_error_map"]).max()) <= 2e-3 and float(np.abs(N(emap)[~c["gt_mask"]]).max(initial=0.0)) == 0.0
        # aligned albedo
        aligned, ratio = M.align_albedo(T(c["albedo"]), T(c["pred_albedo"]), gm)
        r, a = N(ratio), N(aligned)
        dr = np.abs(r.astype(np.float64) - c["ref_ratio"].astype(np.float64))
        print(name, "ratio difference to the reference's in ulp", (dr / ulp32(c["ref_ratio"])).tolist())
        bound = dr[None, :] * c["pred_albedo"].astype(np.float64) + np.where(dr[None, :] > 0, ulp32(np.maximum(c["ref_aligned"], a)), 0.0)
        assert bool((np.abs(a.astype(np.float64) - c["ref_aligned"]) <= bound).all())
        assert float(np.abs(a[~c["gt_mask"]]).max(initial=0.0)) == 0.0 and a.min() >= 0.0 and a.max() <= 1.0
        with_ref_ratio, _ = M.align_albedo(T(c["albedo"]), T(c["pred_albedo"]), gm, ratio=T(c["ref_ratio"]))
        assert np.array_equal(N(with_ref_ratio), c["ref_aligned"])                # the same float32 ratio: identical map
        psnr = M.PSNR()(T(c["ref_aligned"]), T(c["albedo"]), valid_mask=gm)
        assert abs(float(psnr) - float(c["ref_albedo_psnr"])) <= 5e-5


def _all_metrics(M, c):
    H, W = int(c["H"]), int(c["W"])
    gm = T(c["gt_mask"])
    vm = T(c["valid_mask"]) if "valid_mask" in c else None
    img = lambda a: T(a).reshape(H, W, 3)      # noqa: E731
    out = []
    sums, psnr = M.squared_error(T(c["pred_rgb"]), T(c["rgb"]), vm)
    out += [sums, psnr._buf]
    sums, ratio = M.albedo_sums(T(c["albedo"]), T(c["pred_albedo"]), gm)
    out += [sums, ratio._buf, M.align_albedo(T(c["albedo"]), T(c["pred_albedo"]), gm, ratio=ratio)[0]]
    ne = M.normal_error(T(c["pred_normal"]), T(c["normal"]), gm, w2c=T(c["w2c"]), transform=True, normalize=True, want_map=True, want_camera=True)
    out += [ne["sums"], ne["mean"]._buf, ne["map"], ne["camera"], M.mask_rect(gm.reshape(H, W))]
    out += [M.SSIM()(img(c["pred_rgb"]), img(c["rgb"]), valid_mask=gm.reshape(H, W))._buf, M.SSIM()(img(c["pred_rgb"]), img(c["rgb"]))._buf]
    return [o.as_subclass(torch.Tensor) for o in out]


def test_every_metric_is_deterministic_across_calls_and_streams(E):
    from intrinsicavatar_amd import metrics as M
    for name in names(E):
        c = case(E, name)
        first = _all_metrics(M, c)
        second = _all_metrics(M, c)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            third = _all_metrics(M, c)                      # inputs uploaded and kernels launched on a second stream
        side.synchronize()
        for i, (a, b, d) in enumerate(zip(first, second, third)):
            assert N(a).tobytes() == N(b).tobytes(), (name, i)
            assert N(a).tobytes() == N(d).tobytes(), (name, i, "second stream")
