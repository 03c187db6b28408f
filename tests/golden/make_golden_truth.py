"""Golden vectors for ground-truth frames (the RANA and SyntheticHuman datasets: albedo, normal, valid mask, w2c, per-frame HDRI).

Runs ONLY where the reference checkout exists (make_golden_data.REF).  It imports the reference's own datasets/rana.py, datasets/synthetichuman.py and utils/sampler.py
by file path and runs their code on the CPU, with the stubs of make_golden_data.py (cv2.erode / cv2.dilate through `morph`, cv2.imread
through PIL, hydra.utils.instantiate, np.random.randint replayed from recorded words) and three more:
    cv2.boundingRect           (x, y, w, h) of the non-zero pixels, (0, 0, 0, 0) if there are none
    cv2.resize(fx = fy = 1/s)  the centre-2x2 rule for an even integer s that divides both sides: the default INTER_LINEAR samples midway
                               between source pixels s*d + s/2 - 1 and s*d + s/2 on both axes; uint8: (a + b + c + d + 2) >> 2 (the
                               fixed-point path with weights 1024/2048), floating point: ((a + b) + (c + d)) * 0.25 in the array's type
    cv2.imread of a .hdr       through io_formats.load_hdr
What OpenCV really does (anchor of an even kernel, border, the rounding of its resize, IPP-backed builds) is taken from its
documentation and source formula, not from a run.  The datasets hard-code their dilate kernels (100 and 50); on 20 x 24 images those cover
the whole frame, so the modules' np.ones is patched to give k = 5 (RANA) and k = 4 (SyntheticHuman) for the datum cases; the rectangle
sets use the real sizes as well.
    python tests/golden/make_golden_truth.py     ->  tests/golden/golden_truth.npz, tests/golden/truth_parity_bars.json   (data only)
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden_data as MD      # noqa: E402

REF = MD.REF
RECT_KS = (1, 4, 5, 50, 100)
DATUM_K = {"rana": 5, "synthetichuman": 4}
SAMPLER = {"_target_": "utils.sampler.EdgeSampler", "num_sample": 10, "ratio_mask": 0.6, "ratio_edge": 0.3, "kernel_size": 5}


def bounding_rect(img):
    ys, xs = np.nonzero(img)
    if len(xs) == 0:
        return 0, 0, 0, 0
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def center_resize(img, dsize=None, fx=None, fy=None):
    assert dsize is None and fx == fy
    s = int(round(1 / fx))
    H, W = img.shape[:2]
    assert 1 / s == fx and s % 2 == 0 and H % s == 0 and W % s == 0
    lo = s // 2 - 1
    a, b, c, d = img[lo::s, lo::s], img[lo::s, lo + 1::s], img[lo + 1::s, lo::s], img[lo + 1::s, lo + 1::s]
    if img.dtype == np.uint8:
        return ((a.astype(np.int32) + b + c + d + 2) >> 2).astype(np.uint8)
    assert img.dtype.kind == "f"
    return ((a + b) + (c + d)) * img.dtype.type(0.25)


class PatchedOnes:
    """the dataset modules' `np`: numpy, except that the hard-coded (100, 100) / (50, 50) dilate kernel becomes (k, k) when k is set"""

    def __init__(self):
        self.k = None
        self.mod = types.ModuleType("numpy_with_patched_dilate_kernel")
        self.mod.__dict__.update({k: v for k, v in np.__dict__.items() if not k.startswith("__")})
        self.mod.ones = self.ones

    def ones(self, shape, dtype=None):
        if self.k is not None and tuple(np.atleast_1d(shape)) in ((100, 100), (50, 50)):
            shape = (self.k, self.k)
        return np.ones(shape, dtype)


def load_reference():
    sampler, _, words = MD.load_reference()
    from intrinsicavatar_amd import io_formats
    cv2 = sys.modules["cv2"]
    cv2.dilate = lambda img, kernel, iterations=1: MD.morph(img, kernel, np.maximum)
    cv2.boundingRect = bounding_rect
    cv2.resize = center_resize
    cv2.IMREAD_ANYDEPTH, cv2.IMREAD_COLOR = 2, 1
    cv2.imread = lambda path, flags=None: (io_formats.load_hdr(path)[..., ::-1] if path.endswith(".hdr")
                                            else np.asarray(Image.open(path).convert("RGB"))[..., ::-1])
    import importlib.util
    mods, ones = {}, PatchedOnes()
    for name in ("rana", "synthetichuman"):
        spec = importlib.util.spec_from_file_location(f"refdata.{name}", f"{REF}/datasets/{name}.py")
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[f"refdata.{name}"] = mods[name]
        spec.loader.exec_module(mods[name])
        mods[name].np = ones.mod
    return sampler, mods, words, ones


def camera(H, W, seed):
    """float32-representable K and extrinsic of a rotated, translated camera looking at the subject"""
    K = np.array([[37.3 * W / 24, 0.21, 13.7 * W / 24], [0, 35.9 * H / 20, 8.2 * H / 20], [0, 0, 1]])
    ax, ay, az = 0.2 + 0.1 * seed, -0.4, 0.3
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    RT = np.eye(4)
    RT[:3, :3] = Rz @ Ry @ Rx
    RT[:3, 3] = [0.31, -0.2, 2.9 + seed]
    return K.astype(np.float32).astype(np.float64), RT.astype(np.float32).astype(np.float64)


def masks_for(H, W, dtype):
    """[4,H,W]: a blob touching the top-left corner, fractional values only plus a single 1.0 pixel, empty, a blob near the bottom right"""
    m = np.zeros((4, H, W), np.float64)
    m[0] = MD.blob(H, W, 0.15 * W, 0.2 * H, 0.3 * W, 0.35 * H)
    assert m[0, 0, 0] == 1 and m[0, :, -1].max() == 0 and m[0, -1].max() == 0
    m[1] = MD.blob(H, W, 0.55 * W, 0.5 * H, 0.2 * W, 0.25 * H) * 0.5
    m[1, int(0.45 * H), int(0.6 * W)] = 1.0
    m[1, int(0.3 * H), int(0.5 * W)] = 0.25
    m[3] = MD.blob(H, W, 0.8 * W, 0.85 * H, 0.12 * W, 0.1 * H)
    if dtype == np.uint8:
        m[1] = np.where(m[1] > 0, 1, 0)                            # (no fractions in an integer file: a second, smaller blob)
    return m.astype(dtype)


def write_hdr(path, rng):
    from intrinsicavatar_amd import io_formats
    io_formats.save_hdr(path, (rng.random((4, 8, 3)) * 6).astype(np.float32))
    return np.frombuffer(open(path, "rb").read(), np.uint8)


def write_dataset(kind, data_root, subject, H, W, rng, mask_dtype, out, tag):
    """a three-frame subject of `kind` under data_root (both splits) + its HDRIs; the arrays the tests rewrite it from go to out[tag_*]"""
    K, RT = camera(H, W, 0 if kind == "rana" else 1)
    cam = {"intrinsic": K.tolist(), "extrinsic": RT.tolist(), "height": H, "width": W}
    masks = masks_for(H, W, mask_dtype)[:3]
    files = {"images": np.stack([MD.image(H, W, s + 1) for s in range(3)]), "albedos": np.stack([MD.image(H, W, s + 7) for s in range(3)]),
             "normals": np.stack([MD.image(H, W, s + 13) for s in range(3)]),
             "images_relit": np.stack([MD.image(H, W, s + 21) for s in range(3)])}
    thetas = rng.normal(size=(3, 72)) * 0.2
    transl = rng.normal(size=(3, 3)) * 0.1 + np.array([0.0, 0.2, 2.6])
    betas = rng.normal(size=(1, 10))
    hdri_names = ["a.hdr", "b.hdr", "a.hdr"]
    os.makedirs(f"{data_root}/hdri", exist_ok=True)
    for name in ("a.hdr", "b.hdr"):
        if f"hdr_{name[0]}" not in out:
            out[f"hdr_{name[0]}"] = write_hdr(f"{data_root}/hdri/{name}", rng)
        else:
            open(f"{data_root}/hdri/{name}", "wb").write(out[f"hdr_{name[0]}"].tobytes())
    roots = [f"{data_root}/{split}/{subject}" for split in ("train", "test")] if kind == "rana" else [f"{data_root}/{subject}"]
    sub = "" if kind == "rana" else "/00"
    names = dict(images="images", albedos="albedos", normals="normals") if kind == "rana" else \
        dict(images="images", albedos="albedos_png", normals="normals_png", images_relit="images_relit")
    for root in roots:
        for key, d in names.items():
            os.makedirs(f"{root}/{d}{sub}")
            for i in range(3):
                Image.fromarray(files[key][i]).save(f"{root}/{d}{sub}/{i:06d}.png")
        os.makedirs(f"{root}/masks{sub}")
        for i in range(3):
            np.save(f"{root}/masks{sub}/{i:06d}.npy", masks[i])
        os.makedirs(f"{root}/poses")
        with open(f"{root}/cameras.json", "w") as f:
            json.dump(cam if kind == "rana" else {"all_cam_names": ["00"], "00": cam}, f)
        with open(f"{root}/hdri_files.json", "w") as f:
            json.dump(hdri_names, f)
        # train: the optimised file poses/anim_nerf_train.npz ("thetas" layout); test: no cached file, poses.npz sliced by start:end:skip
        np.savez(f"{root}/poses/anim_nerf_train.npz", betas=betas, thetas=thetas, transl=transl)
        np.savez(f"{root}/poses.npz", betas=betas * 0.5, body_pose=thetas[:, 3:] * 2, global_orient=thetas[:, :3] * 2, transl=transl + 0.01)
    out.update({f"{tag}_in_{k}": v for k, v in files.items() if k in names})
    out.update({f"{tag}_in_masks": masks, f"{tag}_in_K": K, f"{tag}_in_RT": RT, f"{tag}_in_hw": np.array([H, W]), f"{tag}_in_betas": betas,
                f"{tag}_in_thetas": thetas, f"{tag}_in_transl": transl, f"{tag}_in_hdri_names": np.array(hdri_names)})


def record_host(out, tag, ds, with_hdri):
    base = lambda paths: np.array([os.path.basename(p) for p in paths])      # noqa: E731
    out.update({f"{tag}_host_img": base(ds.img_lists), f"{tag}_host_albedo": base(ds.albedo_lists), f"{tag}_host_normal": base(ds.normal_lists),
                f"{tag}_host_msk": base(ds.msk_lists), f"{tag}_host_img_dir": np.array(os.path.basename(os.path.dirname(ds.img_lists[0]))),
                f"{tag}_host_img_wh": np.array(ds.img_wh), f"{tag}_host_w2c": ds.w2c})
    out.update({f"{tag}_host_{k}": v for k, v in ds.smpl_params.items()})
    if with_hdri:
        out[f"{tag}_host_hdri"] = base(ds.hdri_files)


def with_indices(ds, seen):
    """the reference's sampler does not return the pixels it drew: hand it np.arange as one more array and take that column off again"""
    inner = ds.sampler.sample

    def sample(mask, *args):
        res = inner(mask, *args, np.arange(mask.size))
        seen.append(res[-1].reshape(-1).astype(np.int64))
        return res[:-1]
    ds.sampler.sample = sample


def build_harness(directory):
    so = os.path.join(directory, "libtruth_harness.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-fvisibility=hidden", "-o", so,
                           os.path.join(ROOT, "tests", "truth_harness.c"), "-lm"])
    return C.CDLL(so)


def host_rays(h, K, c2w, H, W):
    from intrinsicavatar_amd import data
    o, d = np.zeros((H * W, 3), np.float32), np.zeros((H * W, 3), np.float32)
    h.truth_h_rays(C.c_int64(H * W), C.c_int(W), data.camera_words(K, c2w), C.c_void_p(o.ctypes.data), C.c_void_p(d.ctypes.data))
    return o, d


def main():
    sampler, mods, words, ones = load_reference()
    classes = {"rana": mods["rana"].RANADataset, "synthetichuman": mods["synthetichuman"].SyntheticHumanDataset}
    rng = np.random.default_rng(2025)
    out = {}
    cv2 = sys.modules["cv2"]

    # 1. the valid rectangle as the datasets form it, for every mask and k (real sizes 100 and 50 included)
    for H, W in ((20, 24), (150, 130)):
        m = masks_for(H, W, np.float32)
        out[f"rect_masks_{H}x{W}"] = m
        for k in RECT_KS:
            out[f"rect_{H}x{W}_k{k}"] = np.array([cv2.boundingRect(cv2.dilate(f.astype(np.uint8), np.ones((k, k), np.uint8), iterations=1))
                                                  for f in m], np.int32)
        assert (out[f"rect_{H}x{W}_k1"][2] == 0).all() and out[f"rect_{H}x{W}_k1"][1].tolist()[2:] == [1, 1]

    # 2. the datum of both datasets on three-frame subjects of 20 x 24 (H x W)
    tmp = tempfile.mkdtemp(prefix="golden_truth_")
    bars = {}
    harness = build_harness(tmp)
    out["words"] = rng.integers(0, 2 ** 63 - 1, (2, 10), dtype=np.int64)
    for kind in ("rana", "synthetichuman"):
        tag = kind
        root = f"{tmp}/{kind}"
        write_dataset(kind, root, "subject", 20, 24, rng, np.float64, out, tag)
        ones.k = DATUM_K[kind]
        # train mode: EdgeSampler, 10 samples, kernel 5; near / far by the dataset's own rule; frames 0 and 1 (the sampler raises on 2)
        ds = classes[kind](root, "subject", "train", MD.Config(downscale=1, start=0, end=2, skip=1, sampler=SAMPLER, near=None, far=None), mode="train")
        record_host(out, f"{tag}_train", ds, False)
        seen = []
        with_indices(ds, seen)
        for idx in range(2):
            words.queue = list(np.split(out["words"][idx], [ds.sampler.num_mask, ds.sampler.num_mask + ds.sampler.num_edge]))
            datum = ds[idx]
            assert not words.queue
            out.update({f"{tag}_train_{idx}_{k}": np.asarray(v) for k, v in datum.items()})
            out[f"{tag}_train_{idx}_pixel_indices"] = seen[idx]
        words.queue = list(np.split(out["words"][0], [ds.sampler.num_mask, ds.sampler.num_mask + ds.sampler.num_edge]))
        try:
            ds[2]
            raise AssertionError("the reference's sampler must raise on the empty mask")
        except ValueError:
            pass
        # test mode: all three frames, a 4 x 8 .hdr per frame (frames 0 and 2 share a.hdr), the config's near / far
        ds = classes[kind](root, "subject", "test", MD.Config(downscale=1, start=0, end=2, skip=1, near=1.25, far=4.5), mode="test")
        record_host(out, f"{tag}_test", ds, True)
        for idx in range(3):
            out.update({f"{tag}_test_{idx}_{k}": np.asarray(v) for k, v in ds[idx].items()})
        assert not out[f"{tag}_test_2_valid_mask"].any() and 0 < out[f"{tag}_test_0_valid_mask"].sum() < 20 * 24
        # rays_d: the reference's float32 arithmetic against the header's fp64 (host replay), measured on this fixture
        K, RT = out[f"{tag}_in_K"].astype(np.float32), out[f"{tag}_in_RT"].astype(np.float32)
        o, d = host_rays(harness, K, np.linalg.inv(RT), 20, 24)
        assert np.array_equal(o, out[f"{tag}_test_0_rays_o"])
        bars[f"{kind}_rays_d_host_max_abs"] = float(np.abs(d.astype(np.float64) - out[f"{tag}_test_0_rays_d"]).max())

        # 3. downscale = 2 on a 40 x 48 source, every pixel (mode "val": no sampler); masks float64 (RANA) / uint8 (SyntheticHuman)
        ones.k = None                                              # the real kernel: 100 / 50
        root2 = f"{tmp}/{kind}_ds2"
        write_dataset(kind, root2, "subject", 40, 48, rng, np.float64 if kind == "rana" else np.uint8, out, f"{tag}_ds2")
        ds = classes[kind](root2, "subject", "train", MD.Config(downscale=2, start=0, end=2, skip=2, near=None, far=None), mode="val")
        assert ds.img_wh == (24, 20) and len(ds) == 2
        record_host(out, f"{tag}_ds2", ds, False)
        for idx in range(2):
            out.update({f"{tag}_ds2_{idx}_{k}": np.asarray(v) for k, v in ds[idx].items()})
        K, RT = out[f"{tag}_ds2_in_K"].astype(np.float32), out[f"{tag}_ds2_in_RT"].astype(np.float32)
        K[:2] /= 2
        out[f"{tag}_ds2_K"] = K
        _, d = host_rays(harness, K, np.linalg.inv(RT), 20, 24)
        bars[f"{kind}_ds2_rays_d_host_max_abs"] = float(np.abs(d.astype(np.float64) - out[f"{tag}_ds2_0_rays_d"]).max())

    # 4. the downscale rules on their own, s = 2 and 4 on 40 x 48
    src_u8 = np.stack([MD.image(40, 48, 3), MD.image(40, 48, 4)])
    src_f32 = np.stack([masks_for(40, 48, np.float32)[1], rng.random((40, 48)).astype(np.float32)])
    out["down_src_u8"], out["down_src_f32"] = src_u8, src_f32
    for s in (2, 4):
        out[f"down_u8_s{s}"] = np.stack([cv2.resize(f, dsize=None, fx=1 / s, fy=1 / s) for f in src_u8])
        out[f"down_f32_s{s}"] = np.stack([cv2.resize(f, dsize=None, fx=1 / s, fy=1 / s) for f in src_f32])

    bars["rays_d_host_max_abs"] = max(bars.values())
    bars["note"] = ("max |rays_d(host replay of data_math.h, fp64) - rays_d(reference make_rays, float32)| over the fixture's cameras; the "
                    "GPU tests hold the kernel to min(4 x rays_d_host_max_abs, 1e-6)")
    with open(os.path.join(HERE, "truth_parity_bars.json"), "w") as f:
        json.dump(bars, f, indent=1, sort_keys=True)
        f.write("\n")
    path = os.path.join(HERE, "golden_truth.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), len(out), "arrays", bars)
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
