#!/usr/bin/env python3
"""Golden vectors of the animation dataset: the reference's own AnimationDataset (datasets/animation.py:50-206, test split), imported by
file path and run on the CPU, on two small directories.

    python tests/golden/make_golden_animation.py      ->  tests/golden/golden_animation.npz   (data only; needs /root/reference)

Modules the reference imports that are not installed here are stubbed as in make_golden_data.py (datasets.register, pytorch_lightning:
no-ops) plus cv2.imread / cvtColor / resize, which only feed the `hdri` entry: that entry is EXCLUDED from the pin (cv2.resize is not
available here and io_formats.area_resize is this project's own), the stubs hand a constant image through.
Cases:
    aist     the first 12 frames of load/animation/aist (cameras.npz: ONE [4,4] extrinsic, 1080 x 1080), downscale 40 -> 27 x 27 rays,
             frames [2:11:4], near / far from |transl| -+ 1
    perframe the same poses seen by synthetic per-frame extrinsics [12,4,4] with height / width arrays (the reference takes element 0),
             a non-square 480 x 640 frame, downscale 20 -> 24 x 32 rays, frames [1:10:4], near / far given
The camera and pose arrays the directories hold are stored too (`<case>_in_*`): the tests write them back to a directory."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
N_FRAMES = 12


class Config(dict):
    __getattr__ = dict.__getitem__


def load_reference():
    cv2 = types.ModuleType("cv2")
    cv2.IMREAD_ANYDEPTH, cv2.IMREAD_COLOR, cv2.COLOR_BGR2RGB, cv2.INTER_AREA = 2, 1, 4, 3
    cv2.imread = lambda path, flags=None: np.zeros((2, 4, 3), np.float32)
    cv2.cvtColor = lambda img, code: img[..., ::-1]
    cv2.resize = lambda img, size, interpolation=None: np.zeros((size[1], size[0], 3), np.float32)
    pl = types.ModuleType("pytorch_lightning")
    pl.LightningDataModule = object
    datasets = types.ModuleType("datasets")
    datasets.register = lambda name: (lambda cls: cls)
    sys.modules.update({"cv2": cv2, "pytorch_lightning": pl, "datasets": datasets})
    spec = importlib.util.spec_from_file_location("refdata.animation", f"{REF}/datasets/animation.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules["refdata.animation"] = mod
    spec.loader.exec_module(mod)
    return mod


def rot(ax, ay, az):
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def main():
    assert os.path.isdir(REF), "needs /root/reference (build container only)"
    anim = load_reference()
    rng = np.random.default_rng(77)
    src_cam = dict(np.load(f"{REF}/load/animation/aist/cameras.npz"))
    src_pose = dict(np.load(f"{REF}/load/animation/aist/poses.npz"))
    poses, trans = src_pose["poses"][:N_FRAMES], src_pose["trans"][:N_FRAMES]
    betas = rng.normal(size=10)
    ext = np.stack([np.eye(4) for _ in range(N_FRAMES)])
    for f in range(N_FRAMES):                                   # a camera circling the subject, never the identity
        c2w = np.eye(4)
        c2w[:3, :3] = rot(0.05 * f - 0.2, 0.3 * f + 0.1, 0.02 * f)
        c2w[:3, 3] = [0.4 * np.sin(0.3 * f), 0.1 + 0.01 * f, 0.5 * (1 - np.cos(0.3 * f))]
        ext[f] = np.linalg.inv(c2w)
    cases = {
        "aist": (dict(intrinsic=src_cam["intrinsic"], extrinsic=src_cam["extrinsic"], height=src_cam["height"], width=src_cam["width"]),
                 Config(downscale=40, start=2, end=10, skip=4)),
        "perframe": (dict(intrinsic=src_cam["intrinsic"], extrinsic=ext, height=np.full(N_FRAMES, 480), width=np.full(N_FRAMES, 640)),
                     Config(downscale=20, start=1, end=9, skip=4, near=2.5, far=7.5)),
    }
    out = {"betas": betas}
    hdr = os.path.join(tempfile.mkdtemp(prefix="golden_anim_"), "light.hdr")
    open(hdr, "wb").close()
    for tag, (cam, cfg) in cases.items():
        root = tempfile.mkdtemp(prefix="golden_anim_")
        np.savez(f"{root}/cameras.npz", **cam)
        np.savez(f"{root}/poses.npz", poses=poses, trans=trans)
        out.update({f"{tag}_in_cam_{k}": np.asarray(v) for k, v in cam.items()})
        out.update({f"{tag}_in_poses": poses, f"{tag}_in_trans": trans})
        out[f"{tag}_cfg"] = np.array([cfg.downscale, cfg.start, cfg.end, cfg.skip, cfg.get("near") or np.nan, cfg.get("far") or np.nan], np.float64)
        ds = anim.AnimationDataset(root, "subject", "test", cfg, betas=betas, hdri_filepath=hdr)
        out[f"{tag}_len"] = np.array(len(ds))
        out[f"{tag}_img_wh"] = np.array(ds.img_wh)
        for idx in range(len(ds)):
            datum = ds[idx]
            assert datum.pop("hdri").shape == (1024, 2048, 3)
            out.update({f"{tag}_{idx}_{k}": np.asarray(v) for k, v in datum.items()})
        print(tag, "frames", len(ds), "img_wh", ds.img_wh, "keys", sorted(datum))
    path = os.path.join(HERE, "golden_animation.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), len(out), "arrays")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
