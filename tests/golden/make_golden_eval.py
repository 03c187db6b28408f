#!/usr/bin/env python3
"""Golden vectors of frame evaluation (tests/golden/golden_eval.npz), made by running the REFERENCE's own code on the CPU:

    PSNR, NormalError                         /root/reference/systems/criterions.py:43-79      (imported by file path)
    compute_albedo_rescale_factor             /root/reference/models/utils.py:268-277
    IntrinsicAvatarSystem.transform_normals   /root/reference/systems/intrinsic_avatar.py:303-315 (called unbound with a stand-in `self`)
    the aligned-albedo lines                  systems/intrinsic_avatar.py:693-696, on the reference's ratio
    IntrinsicAvatarModel.forward_             with `albedo_only = True`, and with `albedo_align_ratio = (0.8, 0.9, 0.7)`, on the scene, the
                                              RNG recording and the helpers of make_golden_forward.py (imported; that file is untouched)

  python tests/golden/make_golden_eval.py          (build container only: needs /root/reference; CPU, a few minutes)

Only DATA is written: the inputs of four synthetic metric cases, the reference's float32 results, a float64 evaluation of the same
formulas in numpy, the bounding rectangle of every mask by numpy (first / last non-zero row and column: what cv2.boundingRect returns
for a mask), and SSIM.

SSIM is NOT a run of scikit-image: neither scikit-image nor OpenCV is installed where this generator runs.  It is pinned to the
published definition at the version the reference requires (scikit-image 0.18.1, requirements.txt:3) --
structural_similarity(multichannel=True) with its defaults: uniform 7 x 7 window, sample covariance (cov_norm = 49 / 48), K1 = 0.01,
K2 = 0.03, data_range = 2 for float input (the dtype range -1 .. 1), float64 arithmetic, the map cropped by 3 pixels on every side
before the mean, channels averaged -- restated in float64 with scipy.ndimage.uniform_filter, the function scikit-image itself calls
(`ssim_restatement` below).  Two closed-form anchors are stored with it: identical images -> exactly 1.0, and two constant images
a, b -> (2ab + C1) / (a^2 + b^2 + C1) with a, b the float32 pixel values widened to float64.

Condition of the normal fixtures, asserted here: on every pixel the angle between the (transformed, normalised) prediction and the
target lies in [1, 60] degrees, which keeps acos well conditioned (the bar of the GPU test is derived from it)."""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF = "/root/reference"

GF = GB = None                        # make_golden_forward / make_golden_backward: imported by main() (the tests import this file for
                                      # ssim_restatement alone)
N = lambda t: t.detach().cpu().numpy()      # noqa: E731
RATIO = (0.8, 0.9, 0.7)               # albedo_align_ratio of the model runs: components <= 1, so albedo differences cannot grow
MODEL_RUNS = [("light", 16, False), ("uniform_light", 512, True)]
K1, K2, WIN, DATA_RANGE = 0.01, 0.03, 7, 2.0


# ----------------------------------------------------------------------------- SSIM: scikit-image 0.18.1's definition, float64
def ssim_restatement(X, Y):
    """mean SSIM of two [H,W,C] images as structural_similarity(X, Y, multichannel=True) of scikit-image 0.18.1 defines it."""
    from scipy.ndimage import uniform_filter
    assert X.shape == Y.shape and X.ndim == 3 and min(X.shape[:2]) >= WIN
    npix = WIN * WIN
    cov_norm = npix / (npix - 1.0)
    C1, C2 = (K1 * DATA_RANGE) ** 2, (K2 * DATA_RANGE) ** 2
    pad = (WIN - 1) // 2
    vals = []
    for c in range(X.shape[-1]):
        x, y = X[..., c].astype(np.float64), Y[..., c].astype(np.float64)
        ux, uy = uniform_filter(x, size=WIN), uniform_filter(y, size=WIN)
        uxx, uyy, uxy = uniform_filter(x * x, size=WIN), uniform_filter(y * y, size=WIN), uniform_filter(x * y, size=WIN)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
        S = (A1 * A2) / (B1 * B2)
        vals.append(S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean(dtype=np.float64))
    return float(np.mean(np.array(vals, dtype=np.float64)))


def bounding_rect(mask2d):
    """(x, y, w, h) of the non-zero pixels; (0, 0, 0, 0) when there is none."""
    rows, cols = np.nonzero(mask2d.any(1))[0], np.nonzero(mask2d.any(0))[0]
    if rows.size == 0:
        return np.zeros(4, np.int32)
    return np.array([cols[0], rows[0], cols[-1] - cols[0] + 1, rows[-1] - rows[0] + 1], np.int32)


def crop(img, rect):
    x, y, w, h = (int(v) for v in rect)
    return img[y:y + h, x:x + w]


# ----------------------------------------------------------------------------- synthetic frames
def smooth_field(rng, H, W, C, n_waves=6):
    """[H,W,C] in [0,1]: a few random low-frequency waves (an image with structure, so that the window variances are not noise alone)."""
    yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    out = np.zeros((H, W, C))
    for _ in range(n_waves):
        f, ph, amp = rng.uniform(0.5, 4.0, (2, C)), rng.uniform(0, 2 * np.pi, C), rng.uniform(0.3, 1.0, C)
        out += amp * np.sin(2 * np.pi * (f[0] * yy[..., None] + f[1] * xx[..., None]) + ph)
    out = (out - out.min()) / (out.max() - out.min())
    return out


def blob(H, W, cy, cx, ry, rx, lobes, phase, wobble=0.3):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dy, dx = (yy - cy) / ry, (xx - cx) / rx
    r = np.sqrt(dy * dy + dx * dx)
    th = np.arctan2(dy, dx)
    return r < (1.0 - wobble) + wobble * np.sin(lobes * th + phase)


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def make_case(seed, H, W, mask_kind, with_valid_mask):
    rng = np.random.default_rng(seed)
    n = H * W
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    q8 = lambda a: np.round(a * 255.0).astype(np.float32) / np.float32(255.0)      # noqa: E731   (targets come from 8-bit images)
    rgb = q8(smooth_field(rng, H, W, 3)).astype(np.float64)
    pred_rgb = np.clip(rgb + rng.normal(0, 0.04, rgb.shape) + 0.05 * (smooth_field(rng, H, W, 3) - 0.5), 0, 1)
    albedo = q8(0.1 + 0.8 * smooth_field(rng, H, W, 3)).astype(np.float64)
    pred_albedo = np.clip(albedo * np.array([0.7, 1.2, 0.9]) + rng.normal(0, 0.02, albedo.shape), 0, 1)
    if mask_kind == "blob":
        valid = blob(H, W, 0.58 * H, 0.40 * W, 0.27 * H, 0.24 * W, 3, 0.7)
        fg = blob(H, W, 0.56 * H, 0.42 * W, 0.25 * H, 0.22 * W, 5, 2.1)
    else:
        valid, fg = np.ones((H, W), bool), np.ones((H, W), bool)
    alpha = q8(np.where(fg, rng.uniform(0.6, 1.0, (H, W)), rng.uniform(0.0, 0.4, (H, W))))
    # normals: the target has any length; the camera-space prediction is the target's direction turned by 1.5 .. 59 degrees about a random
    # perpendicular axis, scaled; the WORLD-space prediction stored is what transform_normals maps there (flip, then the inverse rotation)
    Rm = rotation(rng)
    tdir = rng.normal(size=(n, 3))
    tdir /= np.linalg.norm(tdir, axis=1, keepdims=True)
    axis = np.cross(tdir, rng.normal(size=(n, 3)))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = np.radians(rng.uniform(1.5, 59.0, n))[:, None]
    pcam = tdir * np.cos(ang) + np.cross(axis, tdir) * np.sin(ang)
    normal = tdir * rng.uniform(0.5, 2.0, (n, 1))
    pcam = pcam * rng.uniform(0.3, 1.2, (n, 1))
    bgpx = ~fg.reshape(n)                             # outside the mask: one constant pair, 30 degrees apart (keeps the file small)
    normal[bgpx], pcam[bgpx] = np.array([0.0, 0.0, 1.5]), np.array([0.0, 0.4, 0.4 * np.sqrt(3.0)])
    pred_normal = (pcam * np.array([1.0, -1.0, -1.0])) @ Rm
    w2c = np.eye(4)
    w2c[:3, :3] = Rm
    w2c[:3, 3] = rng.normal(size=3)
    case = dict(H=np.int32(H), W=np.int32(W), pred_rgb=f32(pred_rgb.reshape(n, 3)), rgb=f32(rgb.reshape(n, 3)),
                pred_albedo=f32(pred_albedo.reshape(n, 3)), albedo=f32(albedo.reshape(n, 3)), alpha=f32(alpha.reshape(n)),
                pred_normal=f32(pred_normal), normal=f32(normal), w2c=f32(w2c[None]))
    if with_valid_mask:
        case["valid_mask"] = valid.reshape(n)
    return case


def evaluate_case(case, crit, utils, sysm):
    """the reference's own float32 results + the float64 evaluation of the same formulas."""
    T = torch.from_numpy
    H, W = int(case["H"]), int(case["W"])
    out = {}
    vm = T(case["valid_mask"]) if "valid_mask" in case else None
    gt_mask = T(case["alpha"]) > 0.5
    m = gt_mask.numpy()
    out["gt_mask"] = m
    # ---- PSNR
    out["ref_psnr"] = N(crit.PSNR()(T(case["pred_rgb"]), T(case["rgb"]), valid_mask=vm))
    d2 = (case["pred_rgb"].astype(np.float64) - case["rgb"].astype(np.float64)) ** 2
    d2 = d2[case["valid_mask"]] if vm is not None else d2
    out["f64_sq_err"], out["f64_sq_count"] = np.float64(d2.sum()), np.int64(d2.size)
    out["f64_psnr"] = np.float64(-10.0 * np.log10(d2.sum() / d2.size))
    # ---- albedo alignment
    ratio = utils.compute_albedo_rescale_factor(T(case["albedo"]), T(case["pred_albedo"]), gt_mask)
    out["ref_ratio"] = N(ratio)
    x, xh = case["albedo"].astype(np.float64)[m], case["pred_albedo"].astype(np.float64)[m]
    out["f64_albedo_sums"] = np.stack([(x * xh).sum(0), (xh * xh).sum(0)], -1)                      # [3, 2]
    out["f64_ratio"] = out["f64_albedo_sums"][:, 0] / out["f64_albedo_sums"][:, 1]
    gt_albedo, pred_albedo = T(case["albedo"]), T(case["pred_albedo"])
    aligned = torch.zeros_like(gt_albedo)
    aligned[gt_mask] = (ratio * pred_albedo[gt_mask]).clamp(min=0.0, max=1.0)
    out["ref_aligned"] = N(aligned)
    out["ref_albedo_psnr"] = N(crit.PSNR()(aligned, gt_albedo, valid_mask=gt_mask))
    da = (N(aligned).astype(np.float64) - case["albedo"].astype(np.float64))[m] ** 2
    out["f64_albedo_psnr"] = np.float64(-10.0 * np.log10(da.sum() / da.size))
    # ---- normals
    batch = dict(w2c=T(case["w2c"]))
    cam = sysm.IntrinsicAvatarSystem.transform_normals(types.SimpleNamespace(rank="cpu"), batch, T(case["pred_normal"]))
    out["ref_normal_cam"] = N(cam)
    NE = crit.NormalError()
    a, b = F.normalize(cam, dim=-1), F.normalize(T(case["normal"]), dim=-1)
    out["ref_normal_error"] = N(NE(a, b, valid_mask=gt_mask))
    out["ref_normal_error_map"] = N(NE(a, b, valid_mask=gt_mask, reduction="none"))
    p64 = (case["pred_normal"].astype(np.float64) @ case["w2c"][0, :3, :3].astype(np.float64).T) * np.array([1.0, -1.0, -1.0])
    t64 = case["normal"].astype(np.float64)
    p64 /= np.maximum(np.linalg.norm(p64, axis=1, keepdims=True), 1e-12)
    t64 /= np.maximum(np.linalg.norm(t64, axis=1, keepdims=True), 1e-12)
    cos = (p64 * t64).sum(-1) / (np.linalg.norm(p64, axis=1) * np.linalg.norm(t64, axis=1) + 1e-8)
    deg = np.degrees(np.arccos(np.clip(cos, -1, 1)))
    assert deg.min() >= 1.0 and deg.max() <= 60.0, (deg.min(), deg.max())          # the fixture's angle condition
    out["f64_normal_error_sum"], out["f64_normal_count"] = np.float64((deg * m).sum()), np.int64(m.sum())
    out["f64_normal_error"] = np.float64((deg * m).sum() / m.sum())
    # ---- rectangles and SSIM
    img = lambda a: a.reshape(H, W, 3)      # noqa: E731
    out["rect_gt"] = bounding_rect(m.reshape(H, W))
    if vm is not None:
        out["rect_valid"] = bounding_rect(case["valid_mask"].reshape(H, W))
        out["f64_rf_ssim"] = np.float64(ssim_restatement(crop(img(case["pred_rgb"]), out["rect_valid"]), crop(img(case["rgb"]), out["rect_valid"])))
    out["f64_rf_ssim_unmasked"] = np.float64(ssim_restatement(img(case["pred_rgb"]), img(case["rgb"])))
    out["f64_albedo_ssim"] = np.float64(ssim_restatement(crop(img(N(aligned)), out["rect_gt"]), crop(img(case["albedo"]), out["rect_gt"])))
    return out


def check_blob_rect(rect, H, W):
    x, y, w, h = (int(v) for v in rect)
    assert x > 0 and y > 0 and x + w < W and y + h < H, ("the rectangle touches an image edge", rect, H, W)
    assert w >= WIN and h >= WIN
    assert abs((x + w / 2) - W / 2) > 0.03 * W and abs((y + h / 2) - H / 2) > 0.03 * H, ("the rectangle is centred", rect, H, W)


# ----------------------------------------------------------------------------- model runs
def model_run(mods, rd, bg, hdri, rays, mode, spp, gi, seed, albedo_only, ratio):
    IA = mods["ia"]
    torch.manual_seed(0)
    with GF.RngLog(seed) as rng:
        GF.RNG = rng
        model = IA.IntrinsicAvatarModel(GF.model_config(mode, spp, gi))
        GF.init_params(model)
        model.eval()
        model.update_step(250, 25000)
        model.train(False)
        assert model.enable_phys and model.importance_sample
        model.background_color = bg
        model.geometry.prepare_bbox(rd.bbox)
        model.radiance.prepare_bbox(rd.bbox)
        model.jitter_materials = False
        model.with_curvature_loss = False
        model.cond = None
        model.prepare_test_occupancy_grid()
        model.emitter.base = nn.Parameter(torch.from_numpy(hdri))
        model.emitter.pdf_scale = (model.emitter.base.shape[0] * model.emitter.base.shape[1]) / (2 * np.pi * np.pi)
        model.emitter.update_pdf()
        model.secondary_rays_d = model.emitter.sample(model.samples_per_pixel)
        model.albedo_only = albedo_only
        if ratio is not None:
            model.albedo_align_ratio = torch.tensor(ratio, dtype=torch.float32)
        with torch.no_grad():
            res = model.forward_(rays.clone())
        log = rng.log
    return res, log, N(model.occupancy_grid_test.binaries), N(model.occupancy_grid_test.aabbs)


def main():
    global GF, GB
    assert os.path.isdir(REF), "needs /root/reference (build container only)"
    import make_golden_forward as GF
    import make_golden_backward as GB
    torch.manual_seed(0)
    mods = GF.import_reference_model()
    tp = sys.modules["lib.torch_pbr"]
    tp.luma = lambda x: ((x[..., 0:1] + x[..., 1:2] + x[..., 2:3]) / 3.0).expand_as(x)
    tp.max_value = lambda x: torch.max(x, dim=-1, keepdim=True)[0].expand_as(x)
    sysm = GB.import_reference_system()
    crit, utils = sys.modules["systems.criterions"], sys.modules["models.utils"]
    out = {}
    # ---- metric cases
    cases = [("blob_96x80", 101, 96, 80, "blob", True), ("blob_61x47", 102, 61, 47, "blob", True), ("full_40x40", 103, 40, 40, "full", True),
             ("nomask_26x24", 104, 26, 24, "blob", False)]
    out["cases"] = np.array([c[0] for c in cases])
    for name, seed, H, W, kind, with_vm in cases:
        case = make_case(seed, H, W, kind, with_vm)
        res = evaluate_case(case, crit, utils, sysm)
        if kind == "blob":
            check_blob_rect(res["rect_gt"], H, W)
            if with_vm:
                check_blob_rect(res["rect_valid"], H, W)
        else:
            assert tuple(res["rect_gt"]) == (0, 0, W, H) and tuple(res["rect_valid"]) == (0, 0, W, H)
        for k, v in {**case, **res}.items():
            out[f"{name}/{k}"] = v
        print(name, {k: (float(v) if np.ndim(v) == 0 else v.tolist()) for k, v in res.items() if np.size(v) <= 6})
    # ---- SSIM anchors
    rng = np.random.default_rng(7)
    same = rng.random((24, 30, 3)).astype(np.float32)
    out["anchor_identical_image"] = same
    out["anchor_identical_ssim"] = np.float64(ssim_restatement(same, same))
    assert out["anchor_identical_ssim"] == 1.0
    a, b = np.float32(0.3), np.float32(0.5)
    ca, cb = np.full((20, 22, 3), a, np.float32), np.full((20, 22, 3), b, np.float32)
    C1 = (K1 * DATA_RANGE) ** 2
    closed = (2 * float(a) * float(b) + C1) / (float(a) ** 2 + float(b) ** 2 + C1)
    out["anchor_constant_ab"] = np.array([a, b], np.float32)
    out["anchor_constant_ssim"] = np.float64(ssim_restatement(ca, cb))
    out["anchor_constant_closed_form"] = np.float64(closed)
    assert abs(out["anchor_constant_ssim"] - closed) <= 1e-12, (out["anchor_constant_ssim"], closed)
    print("anchors", float(out["anchor_identical_ssim"]), float(out["anchor_constant_ssim"]), closed)
    # ---- model runs
    dummy = type("Dummy", (nn.Module,), {"__init__": lambda self, c=None: nn.Module.__init__(self), "forward": lambda self, *a, **k: None})
    registry = mods["registry"]
    registry["none"] = dummy
    wrap, rd, _ = GF.build_rig(mods)
    registry["prebuilt"] = lambda cfg: wrap
    rays = torch.from_numpy(GF.S.camera_rays(GF.HW, GF.HW))
    bg = torch.tensor([0.2, 0.4, 0.6])
    hdri = GF.hdri()
    Gf = np.load(os.path.join(HERE, "golden_forward.npz"))
    assert np.array_equal(Gf["rays"], N(rays)) and np.array_equal(Gf["hdri"], hdri) and np.array_equal(Gf["background_color"], N(bg))
    out["ratio"] = np.array(RATIO, np.float32)
    tags = []
    for mode, spp, gi in MODEL_RUNS:
        base = f"{mode}_{spp}_{'gi' if gi else 'nogi'}"
        for suffix, albedo_only, ratio in (("albedo_only", True, None), ("ratio", False, RATIO)):
            tag = f"{base}_{suffix}"
            res, log, binaries, aabb = model_run(mods, rd, bg, hdri, rays, mode, spp, gi, 2000 + len(tags), albedo_only, ratio)
            # the scene of the run is golden_forward.npz's (same occupancy grid: its jitter is a closed form of the draw's position)
            assert np.array_equal(binaries, Gf[base + "_occ_binaries"]) and np.array_equal(aabb, Gf[base + "_occ_aabb"]), tag
            tags.append(tag)
            out[tag + "_rng_kinds"] = np.array([k for k, _ in log])
            for i, (_, t) in enumerate(log):
                out[f"{tag}_rng_{i}"] = N(t)
            out[tag + "_out_keys"] = np.array(sorted(res.keys()))
            for k, v in res.items():
                out[f"{tag}_out_{k}"] = N(v)
            print(tag, "rng draws:", [(k, tuple(t.shape)) for k, t in log], "n_samples", int(res["num_samples"][0]), flush=True)
    out["model_runs"] = np.array(tags)
    torch.Tensor.cuda, torch.cuda.device = mods["restore"]
    path = f"{HERE}/golden_eval.npz"
    np.savez_compressed(path, **out)
    print("golden_eval.npz", os.path.getsize(path) // 1024, "KiB,", len(out), "arrays")


if __name__ == "__main__":
    main()
