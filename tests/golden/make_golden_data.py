"""Golden vectors for training batches (camera rays, pixel samplers, the dataset datum).

Runs ONLY where /root/reference exists.  It imports the reference's own utils/sampler.py and datasets/peoplesnapshot.py by file path and
runs their code on the CPU; the modules they import that are not installed here are stubbed:
    cv2.erode / cv2.dilate     a plain numpy restatement of the formula OpenCV documents for a rectangular kernel: the minimum / maximum over
                               the kernel's taps at offsets -(k/2) ... k - 1 - k/2 (anchor k/2), taps outside the image ignored (the default
                               border value never wins); a 1-D array of N elements is an N x 1 image (N rows, 1 column)
    cv2.imread / cvtColor      through PIL
    hydra.utils.instantiate    builds the reference's own sampler class from the config mapping
    datasets.register, pytorch_lightning   no-ops (the data module is not used)
    np.random.randint(lo, hi, size)   inside the sampler module only: lo + words[:size] % (hi - lo) over recorded int64 word arrays, one per call
What OpenCV really does at the anchor, the border and for a 1-D array is taken from its documentation, not from a run.
    python tests/golden/make_golden_data.py      ->  tests/golden/golden_data.npz   (data only)
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

WINDOW_LENGTHS = (1, 7, 255, 256, 257, 1961)
WINDOW_KS = (1, 5, 16, 32, 64)


def morph(img, kernel, pick):
    """rectangular erode (pick = np.minimum) / dilate (np.maximum) as documented: dst(y, x) = pick over the kernel's taps (j, i) of
    src(y + j - kh/2, x + i - kw/2), taps outside the image left out."""
    one_d = img.ndim == 1
    a = img.reshape(-1, 1) if one_d else img
    kh, kw = kernel.shape
    H, W = a.shape
    out = a.copy()                                             # the anchor tap itself
    for j in range(kh):
        for i in range(kw):
            dy, dx = j - kh // 2, i - kw // 2
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 < y1 and x0 < x1:
                out[y0:y1, x0:x1] = pick(out[y0:y1, x0:x1], a[y0 + dy:y1 + dy, x0 + dx:x1 + dx])
    return out.reshape(img.shape)


class Words:
    """np.random stand-in of the sampler module: randint(lo, hi, size) -> lo + words % (hi - lo) over the queued arrays, one per call."""

    def __init__(self):
        self.queue = []

    def randint(self, lo, hi, size):
        if hi - lo <= 0:
            raise ValueError("low >= high")
        w = self.queue.pop(0)
        assert w.shape == (size,) and w.dtype == np.int64 and (w >= 0).all()
        return lo + w % (hi - lo)


def load_reference():
    cv2 = types.ModuleType("cv2")
    cv2.erode = lambda img, kernel: morph(img, kernel, np.minimum)
    cv2.dilate = lambda img, kernel: morph(img, kernel, np.maximum)
    cv2.COLOR_BGR2RGB = 4
    cv2.imread = lambda path: np.asarray(Image.open(path).convert("RGB"))[..., ::-1]       # BGR, like OpenCV
    cv2.cvtColor = lambda img, code: img[..., ::-1]
    hydra = types.ModuleType("hydra")
    hydra.utils = types.ModuleType("hydra.utils")
    pl = types.ModuleType("pytorch_lightning")
    pl.LightningDataModule = object
    datasets = types.ModuleType("datasets")
    datasets.register = lambda name: (lambda cls: cls)
    utils = types.ModuleType("utils")
    utils.__path__ = []
    sys.modules.update({"cv2": cv2, "hydra": hydra, "hydra.utils": hydra.utils, "pytorch_lightning": pl, "datasets": datasets, "utils": utils})

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    sampler = load("utils.sampler", f"{REF}/utils/sampler.py")
    utils.sampler = sampler
    words = Words()
    fake_np = types.ModuleType("numpy_with_recorded_draws")       # the sampler module's `np`: numpy, except np.random
    fake_np.__dict__.update({k: v for k, v in np.__dict__.items() if not k.startswith("__")})
    fake_np.random = words
    sampler.np = fake_np
    hydra.utils.instantiate = lambda cfg: getattr(sampler, cfg["_target_"].rsplit(".", 1)[1])(**{k: v for k, v in cfg.items() if k != "_target_"})
    ps = load("refdata.peoplesnapshot", f"{REF}/datasets/peoplesnapshot.py")
    return sampler, ps, words


def cameras():
    """two float64 cameras: a square one looking down -z, and a non-square one with a rotated c2w and the principal point off-centre."""
    K0 = np.array([[1500.0, 0, 270.0], [0, 1500.0, 270.0], [0, 0, 1]])
    c0 = np.eye(4)
    c0[:3, 3] = [0.05, -0.1, 2.5]
    K1 = np.array([[37.3, 0.21, 13.7], [0, 35.9, 8.2], [0, 0, 1]])
    ax, ay, az = 0.3, -0.7, 1.1
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    c1 = np.eye(4)
    c1[:3, :3] = Rz @ Ry @ Rx
    c1[:3, 3] = [0.31, -1.7, 2.9]
    return (K0, c0, 540, 540), (K1, c1, 20, 24)


def window_masks(n, rng):
    """[7, n] float32: zero, one, single one at 0 / at the end, runs shorter than the windows, runs across the 256- and 1024-element tile
    boundaries, non-binary values."""
    m = np.zeros((7, n), np.float32)
    m[1] = 1
    m[2, 0] = 1
    m[3, -1] = 1
    pos = 0
    while pos < n:                                             # runs of 1 .. 12 ones, gaps of 1 .. 40
        run = int(rng.integers(1, 13))
        m[4, pos:pos + run] = 1
        pos += run + int(rng.integers(1, 41))
    m[5, 250:262] = 1
    m[5, 1018:1030] = 1
    m[6] = rng.choice(np.array([0, 0.25, 0.5, 1], np.float32), n, p=[0.55, 0.15, 0.15, 0.15])
    return m


def blob(H, W, cx, cy, rx, ry):
    y, x = np.mgrid[0:H, 0:W]
    return ((((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2) <= 1).astype(np.float32)


def image(H, W, seed):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([(x * 3 + y * 5 + seed * 11) % 256, (x * 7 + y * 2 + 40 * seed) % 256, (x + y * y + seed) % 256], -1).astype(np.uint8)


def run_sampler(words, smp, rec, mask, img_u8, rays_o, rays_d):
    """one reference `sample` call: the draw's words split in call order; the pixel indices come out as a gathered np.arange."""
    n = smp.num_rand + getattr(smp, "num_mask", 0) + getattr(smp, "num_edge", 0)
    cuts = np.cumsum([getattr(smp, "num_mask", 0), getattr(smp, "num_edge", 0)])
    parts = np.split(rec, cuts)
    words.queue = [p for p, present in zip(parts, (hasattr(smp, "num_mask"), hasattr(smp, "num_edge"), True)) if present]
    img = (img_u8[..., :3] / 255).astype(np.float32)          # datasets/peoplesnapshot.py:126
    alpha, rgb, o, d, idx = smp.sample(mask, img, rays_o, rays_d, np.arange(mask.size))
    assert not words.queue and len(alpha) == n
    return dict(alpha=alpha, rgb=rgb, rays_o=o, rays_d=d, indices=idx.reshape(-1).astype(np.int64))


class Config(dict):
    __getattr__ = dict.__getitem__


def write_dataset(root, K, c2w, H, W, rng):
    os.makedirs(f"{root}/images")
    os.makedirs(f"{root}/masks")
    os.makedirs(f"{root}/poses")
    np.savez(f"{root}/cameras.npz", intrinsic=K, extrinsic=np.linalg.inv(c2w), height=H, width=W)
    imgs = np.stack([image(H, W, s + 1) for s in range(3)])
    masks = [blob(H, W, 11, 9, 6.5, 5.2).astype(np.uint8), blob(H, W, 14, 10, 4.2, 7.5).astype(np.float64), blob(H, W, 9, 8, 7, 4).astype(np.uint8)]
    masks[1][8:11, 12:15] = 0.25                               # non-binary values survive astype(np.float32)
    for i in range(3):
        Image.fromarray(imgs[i]).save(f"{root}/images/image_{i:04d}.png")
        np.save(f"{root}/masks/mask_{i:04d}.npy", masks[i])
    thetas = (rng.normal(size=(3, 72)) * 0.2)
    transl = rng.normal(size=(3, 3)) * 0.1 + np.array([0.0, 0.2, 2.6])
    betas = rng.normal(size=(1, 10))
    # train: the optimised file poses/anim_nerf_train.npz ("thetas" layout); test: no cached file, poses.npz sliced by start:end:skip
    np.savez(f"{root}/poses/anim_nerf_train.npz", betas=betas, thetas=thetas, transl=transl)
    np.savez(f"{root}/poses.npz", betas=betas * 0.5, body_pose=thetas[:, 3:] * 2, global_orient=thetas[:, :3] * 2, transl=transl + 0.01)
    files = {"ds_cam_intrinsic": K, "ds_cam_extrinsic": np.linalg.inv(c2w), "ds_images": imgs, "ds_mask0": masks[0], "ds_mask1": masks[1],
             "ds_mask2": masks[2], "ds_train_betas": betas, "ds_train_thetas": thetas, "ds_train_transl": transl,
             "ds_poses_betas": betas * 0.5, "ds_poses_body_pose": thetas[:, 3:] * 2, "ds_poses_global_orient": thetas[:, :3] * 2,
             "ds_poses_transl": transl + 0.01}
    return files


def main():
    sampler, ps, words = load_reference()
    rng = np.random.default_rng(2024)
    out = {}

    # 1. make_rays on the two cameras
    cams = cameras()
    rays = []
    for c, (K, c2w, H, W) in enumerate(cams):
        o, d = ps.make_rays(K, c2w, H, W)
        assert o.dtype == np.float32 and d.shape == (H, W, 3)
        rays.append((o, d))
        out.update({f"cam{c}_K": K, f"cam{c}_c2w": c2w, f"cam{c}_hw": np.array([H, W])})
    out["cam1_rays_o"], out["cam1_rays_d"] = rays[1]                                  # 20 x 24: the whole frame
    sel = np.sort(rng.choice(540 * 540, 4096, replace=False))
    out["cam0_sel"], out["cam0_rays_o"], out["cam0_rays_d"] = sel, rays[0][0].reshape(-1, 3)[sel], rays[0][1].reshape(-1, 3)[sel]

    # 2. the window: the stub's documented formula on flat arrays (N x 1 images) and on 2-D images
    for n in WINDOW_LENGTHS:
        m = window_masks(n, rng)
        out[f"win_in_{n}"] = m
        out[f"win_min_{n}"] = np.stack([np.stack([sys.modules["cv2"].erode(r, np.ones((k, k), np.uint8)) for r in m]) for k in WINDOW_KS])
        out[f"win_max_{n}"] = np.stack([np.stack([sys.modules["cv2"].dilate(r, np.ones((k, k), np.uint8)) for r in m]) for k in WINDOW_KS])
    img2 = {"37x53": window_masks(37 * 53, rng)[4].reshape(37, 53) * window_masks(37 * 53, rng)[6].reshape(37, 53) + blob(37, 53, 30, 17, 9.5, 8),
            "64x64": blob(64, 64, 31.5, 30, 17.3, 17.3)}
    for tag, m in img2.items():
        m = m.astype(np.float32)
        out[f"win2d_in_{tag}"] = m
        out[f"win2d_min_{tag}"] = np.stack([sys.modules["cv2"].erode(m, np.ones((k, k), np.uint8)) for k in WINDOW_KS])
        out[f"win2d_max_{tag}"] = np.stack([sys.modules["cv2"].dilate(m, np.ones((k, k), np.uint8)) for k in WINDOW_KS])

    # 3. the reference's samplers.  big: 540 x 540, the shipped kernel_size 16, 4096 samples; small: 20 x 24 (H x W), 10 samples
    big_mask = np.maximum(blob(540, 540, 260, 290, 95, 210), 0.5 * blob(540, 540, 380, 200, 60, 40)).astype(np.float32)
    small_mask = blob(20, 24, 11, 9, 6.5, 5.2)
    small_mask[9, 10] = 0.25
    frames = {"big": (big_mask, image(540, 540, 0), rays[0]), "small": (small_mask, image(20, 24, 5), rays[1])}
    for tag, (m, im, _) in frames.items():
        out[f"{tag}_mask"], out[f"{tag}_image"] = m, im
    cases = {"big_edge": ("big", sampler.EdgeSampler, dict(num_sample=4096, ratio_mask=0.6, ratio_edge=0.3, kernel_size=16)),
             "big_norand": ("big", sampler.EdgeSampler, dict(num_sample=4096, ratio_mask=0.75, ratio_edge=0.25, kernel_size=16)),
             "big_uniform": ("big", sampler.UniformSampler, dict(num_sample=4096)),
             "small_edge": ("small", sampler.EdgeSampler, dict(num_sample=10, ratio_mask=0.6, ratio_edge=0.3, kernel_size=5)),
             "small_norand": ("small", sampler.EdgeSampler, dict(num_sample=10, ratio_mask=0.7, ratio_edge=0.3, kernel_size=5)),
             "small_uniform": ("small", sampler.UniformSampler, dict(num_sample=10))}
    for name, (tag, cls, kw) in cases.items():
        smp = cls(**kw)
        m, im, (ro, rd) = frames[tag]
        rec = rng.integers(0, 2 ** 63 - 1, kw["num_sample"], dtype=np.int64)
        res = run_sampler(words, smp, rec, m, im, ro, rd)
        out[f"{name}_words"] = rec
        out[f"{name}_split"] = np.array([getattr(smp, "num_mask", 0), getattr(smp, "num_edge", 0), smp.num_rand])
        out.update({f"{name}_{k}": v for k, v in res.items()})
    assert out["big_norand_split"][2] == 0 and out["small_norand_split"][2] == 0
    # the lists themselves (np.where of the reference's expressions) for three frames, one of them empty
    list_masks = np.stack([small_mask, np.zeros_like(small_mask), blob(20, 24, 5, 14, 9, 3)])
    out["lists_masks"] = list_masks
    for f, m in enumerate(list_masks):
        flat = m.reshape(-1)
        k5 = np.ones((5, 5), np.uint8)
        mask_e = sys.modules["cv2"].dilate(flat, k5) - sys.modules["cv2"].erode(flat, k5)
        out[f"lists_mask_loc_{f}"], out[f"lists_edge_loc_{f}"] = np.where(flat)[0], np.where(mask_e)[0]

    # 4. PeopleSnapshotDataset.__getitem__ on a three-frame directory (20 x 24 images), train and test mode
    K, c2w, H, W = cams[1]
    tmp = tempfile.mkdtemp(prefix="golden_data_")
    out.update(write_dataset(tmp, K, c2w, H, W, rng))
    smp_cfg = {"_target_": "utils.sampler.EdgeSampler", "num_sample": 10, "ratio_mask": 0.6, "ratio_edge": 0.3, "kernel_size": 5}
    out["ds_words"] = rng.integers(0, 2 ** 63 - 1, (3, 10), dtype=np.int64)
    for tag, near, far in (("cfg", 1.25, 4.5), ("transl", None, None)):
        ds = ps.PeopleSnapshotDataset(tmp, "subject", "train", Config(downscale=1, start=0, end=2, skip=1, sampler=smp_cfg, near=near, far=far),
                                      mode="train")
        for idx in range(3):
            words.queue = list(np.split(out["ds_words"][idx], [ds.sampler.num_mask, ds.sampler.num_mask + ds.sampler.num_edge]))
            datum = ds[idx]
            assert not words.queue
            out.update({f"ds_train_{tag}_{idx}_{k}": np.asarray(v) for k, v in datum.items()})
    # test split: frames 0 and 2 (start 0, end 2, skip 2), no optimised pose file -> poses.npz sliced
    ds = ps.PeopleSnapshotDataset(tmp, "subject", "test", Config(downscale=1, start=0, end=2, skip=2), mode="test")
    assert len(ds) == 2
    for idx in range(2):
        out.update({f"ds_test_{idx}_{k}": np.asarray(v) for k, v in ds[idx].items()})

    path = os.path.join(HERE, "golden_data.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), len(out), "arrays")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
