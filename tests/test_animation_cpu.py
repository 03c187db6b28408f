"""CPU: the host-only part of data.AnimationFrames (data.animation_host: file parsing, K, translation, near / far) against the reference's
own AnimationDataset, test split (tests/golden/golden_animation.npz, written by tests/golden/make_golden_animation.py).  The rays and the
datum on the device: tests/test_gpu_emitter_background.py."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("aist", "perframe")


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "golden_animation.npz"))


def write_case(G, tag, root):
    """the directory the fixture was made from: cameras.npz and poses.npz"""
    np.savez(os.path.join(root, "cameras.npz"), **{k: G[f"{tag}_in_cam_{k}"] for k in ("intrinsic", "extrinsic", "height", "width")})
    np.savez(os.path.join(root, "poses.npz"), poses=G[f"{tag}_in_poses"], trans=G[f"{tag}_in_trans"])
    ds, start, end, skip, near, far = G[f"{tag}_cfg"]
    return dict(start=int(start), end=int(end), skip=int(skip), downscale=int(ds), near=None if np.isnan(near) else float(near),
                far=None if np.isnan(far) else float(far))


@pytest.mark.parametrize("tag", CASES)
def test_host_part_against_the_references_dataset(G, tag, tmp_path):
    from intrinsicavatar_amd import data
    kw = write_case(G, tag, str(tmp_path))
    h = data.animation_host(str(tmp_path), G["betas"], **kw)
    F = int(G[f"{tag}_len"])
    assert len(h["global_orient"]) == F == 3
    assert (h["width"], h["height"]) == tuple(int(v) for v in G[f"{tag}_img_wh"])
    assert h["per_frame_extrinsic"] == (tag == "perframe")
    n = h["width"] * h["height"]
    for idx in range(F):
        ref = {k: G[f"{tag}_{idx}_{k}"] for k in ("betas", "global_orient", "body_pose", "transl", "index", "w2c", "near", "far")}
        assert int(ref["index"]) == idx
        for k, got in (("betas", h["betas"][0]), ("global_orient", h["global_orient"][idx]), ("body_pose", h["body_pose"][idx]),
                       ("transl", h["transl"][idx]), ("w2c", h["w2c"][idx])):
            assert got.dtype == ref[k].dtype == np.float32 and np.array_equal(got, ref[k]), (k, idx)
        for k in ("near", "far"):            # the reference's [HW] arrays are one number per frame
            assert ref[k].shape == (n,) and ref[k].dtype == np.float32
            assert np.array_equal(np.full(n, h[k][idx], np.float32), ref[k]), (k, idx)


def test_intrinsics_as_the_reference_writes_them(G, tmp_path):
    """K = diag(2000, 2000, 1), principal point (height // 2, width // 2) IN THAT ORDER, K[:2] /= downscale; per-frame cameras: height and
    width are arrays and element 0 counts"""
    from intrinsicavatar_amd import data
    kw = write_case(G, "perframe", str(tmp_path))
    h = data.animation_host(str(tmp_path), G["betas"], **kw)
    assert (h["height"], h["width"]) == (24, 32)
    assert np.array_equal(h["K"], np.array([[100.0, 0, 12.0], [0, 100.0, 16.0], [0, 0, 1.0]]))            # 240 / 20 (from the HEIGHT), 320 / 20
    kw1 = dict(kw, downscale=1)
    h1 = data.animation_host(str(tmp_path), G["betas"], **kw1)
    assert (h1["height"], h1["width"]) == (480, 640) and h1["K"][0, 2] == 240 and h1["K"][1, 2] == 320 and h1["K"][0, 0] == 2000


def test_translation_slice_and_near_far(G, tmp_path):
    from intrinsicavatar_amd import data
    kw = write_case(G, "aist", str(tmp_path))
    h = data.animation_host(str(tmp_path), G["betas"], **kw)
    trans = G["aist_in_trans"]
    want = trans - trans[0:1]
    want += (0, 0.15, 5)                                         # in place on float32, as the reference writes it
    want = want[kw["start"]:kw["end"] + 1:kw["skip"]]
    assert np.array_equal(h["transl"], want)
    dist = np.sqrt(np.square(h["transl"]).sum(-1))
    assert np.array_equal(h["near"], (dist - 1).astype(np.float32)) and np.array_equal(h["far"], (dist + 1).astype(np.float32))
    hc = data.animation_host(str(tmp_path), G["betas"], **dict(kw, near=0.5, far=9.0))
    assert np.array_equal(hc["near"], np.full(3, 0.5, np.float32)) and np.array_equal(hc["far"], np.full(3, 9.0, np.float32))
    # a single extrinsic is repeated per frame
    assert h["w2c"].shape == (3, 4, 4) and np.array_equal(h["w2c"][0], h["w2c"][2])


def test_frames_need_a_gpu(G, tmp_path):
    from intrinsicavatar_amd import data, _lib
    kw = write_case(G, "aist", str(tmp_path))
    with pytest.raises(_lib.IaError):
        data.AnimationFrames.from_dir(str(tmp_path), G["betas"], device="cpu", **kw)
