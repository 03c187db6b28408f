"""Ground-truth frames without a GPU: the additions to intrinsicavatar_amd/csrc/data_math.h replayed on the host by tests/truth_harness.c,
and data.truth_host, against tests/golden/golden_truth.npz (the reference's own RANADataset / SyntheticHumanDataset with cv2 stubbed by the
documented formulas, tests/golden/make_golden_truth.py).

Everything is bit for bit except the ray directions: the reference forms them in float32, the header in fp64 with one rounding at the
end.  The difference of the host replay is measured here on the fixture's cameras and must be the value recorded in
tests/golden/truth_parity_bars.json, from which the GPU tests take their bound (4 x, never above 1e-6)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "golden_truth.npz")
BARS = os.path.join(HERE, "golden", "truth_parity_bars.json")
KINDS = ("rana", "synthetichuman")
RECT_KS = (1, 4, 5, 50, 100)
RECT_SIZES = ((20, 24), (150, 130))
DATUM_K = {"rana": 5, "synthetichuman": 4}          # the dilate kernel the fixture's datum cases were recorded with

vp = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731


def build_harness(directory):
    so = os.path.join(str(directory), "libtruth_harness.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-fvisibility=hidden", "-o", so,
                           os.path.join(HERE, "truth_harness.c"), "-lm"])
    return C.CDLL(so)


def load_golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def dir_bound():
    """the GPU's bound on rays_d: 4 x the host replay's measured difference (the margin is for the summation order of the reference's
    BLAS), never above 1e-6"""
    return min(4 * json.load(open(BARS))["rays_d_host_max_abs"], 1e-6)


def write_dataset(data_root, g, kind, tag):
    """the fixture's subject `tag` ("rana", "rana_ds2", ...) written from its arrays, both splits; -> data_root"""
    from PIL import Image
    rana = kind == "rana"
    H, W = (int(v) for v in g[f"{tag}_in_hw"])
    cam = {"intrinsic": g[f"{tag}_in_K"].tolist(), "extrinsic": g[f"{tag}_in_RT"].tolist(), "height": H, "width": W}
    os.makedirs(os.path.join(data_root, "hdri"), exist_ok=True)
    for name in ("a", "b"):
        with open(os.path.join(data_root, "hdri", f"{name}.hdr"), "wb") as f:
            f.write(g[f"hdr_{name}"].tobytes())
    roots = [os.path.join(data_root, split, "subject") for split in ("train", "test")] if rana else [os.path.join(data_root, "subject")]
    names = dict(images="images", albedos="albedos", normals="normals") if rana else \
        dict(images="images/00", albedos="albedos_png/00", normals="normals_png/00", images_relit="images_relit/00")
    betas, thetas, transl = g[f"{tag}_in_betas"], g[f"{tag}_in_thetas"], g[f"{tag}_in_transl"]
    for root in roots:
        for key, d in names.items():
            os.makedirs(os.path.join(root, d))
            for i in range(3):
                Image.fromarray(g[f"{tag}_in_{key}"][i]).save(os.path.join(root, d, f"{i:06d}.png"))
        mdir = os.path.join(root, "masks" if rana else "masks/00")
        os.makedirs(mdir)
        for i in range(3):
            np.save(os.path.join(mdir, f"{i:06d}.npy"), g[f"{tag}_in_masks"][i])
        os.makedirs(os.path.join(root, "poses"))
        with open(os.path.join(root, "cameras.json"), "w") as f:
            json.dump(cam if rana else {"all_cam_names": ["00"], "00": cam}, f)
        with open(os.path.join(root, "hdri_files.json"), "w") as f:
            json.dump([str(s) for s in g[f"{tag}_in_hdri_names"]], f)
        np.savez(os.path.join(root, "poses", "anim_nerf_train.npz"), betas=betas, thetas=thetas, transl=transl)
        np.savez(os.path.join(root, "poses.npz"), betas=betas * 0.5, body_pose=thetas[:, 3:] * 2, global_orient=thetas[:, :3] * 2,
                 transl=transl + 0.01)
    return str(data_root)


def collated(v):
    """what the DataLoader's default collate makes of one datum entry at batch_size 1"""
    v = np.asarray(v)
    if v.ndim == 0:
        v = v.astype(np.int64 if v.dtype.kind == "i" else np.float64)
    return v[None]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("truth"))


@pytest.fixture(scope="module")
def g():
    return load_golden()


@pytest.fixture(scope="module")
def roots(g, tmp_path_factory):
    base = tmp_path_factory.mktemp("truth_sets")
    return {tag: write_dataset(str(base / tag), g, tag.split("_")[0], tag) for kind in KINDS for tag in (kind, f"{kind}_ds2")}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def h_rect(h, masks, k):
    masks = np.ascontiguousarray(masks, np.float32)
    F, H, W = masks.shape
    rect = np.zeros((F, 4), np.int32)
    h.truth_h_valid_rect(C.c_int64(F), C.c_int(H), C.c_int(W), vp(masks), C.c_int(k), vp(rect))
    return rect


def h_valid(h, H, W, rect):
    rect = np.ascontiguousarray(rect, np.int32)
    out = np.zeros(H * W, np.uint8)
    h.truth_h_valid_mask(C.c_int(H), C.c_int(W), vp(rect), vp(out))
    return out.astype(bool)


def h_down(h, x, s):
    x = np.ascontiguousarray(x)
    F, H, W = x.shape[:3]
    out = np.zeros((F, H // s, W // s) + x.shape[3:], x.dtype)
    if x.dtype == np.uint8:
        h.truth_h_downscale_u8(C.c_int64(F), C.c_int(H), C.c_int(W), C.c_int(x.shape[3] if x.ndim == 4 else 1), C.c_int(s), vp(x), vp(out))
    else:
        h.truth_h_downscale_f32(C.c_int64(F), C.c_int(H), C.c_int(W), C.c_int(s), vp(x), vp(out))
    return out


def test_decode_tables_bit_identical(harness, g):
    albedo, normal = np.zeros(256, np.float32), np.zeros(256, np.float32)
    harness.truth_h_decode_tables(vp(albedo), vp(normal))
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(bits(albedo), bits((v / 255).astype(np.float32)))
    assert np.array_equal(bits(normal), bits(((v / 255).astype(np.float32) - 0.5) * 2))
    # and through the reference's own datum: every pixel of test frame 0
    for kind in KINDS:
        assert np.array_equal(bits(albedo[g[f"{kind}_in_albedos"][0].reshape(-1, 3)]), bits(g[f"{kind}_test_0_albedo"]))
        assert np.array_equal(bits(normal[g[f"{kind}_in_normals"][0].reshape(-1, 3)]), bits(g[f"{kind}_test_0_normal"]))


def test_which_mask_pixels_count(harness):
    """msk.astype(np.uint8) != 0 on [0, 256)"""
    vals = np.array([0, 0.25, 0.5, 0.999999, 1, 1.5, 2, 255, 255.9], np.float32)
    got = [harness.truth_h_mask_counts(C.c_float(float(v))) for v in vals]
    assert got == (vals.astype(np.uint8) != 0).astype(int).tolist()
    assert got == [0, 0, 0, 0, 1, 1, 1, 1, 1]


@pytest.mark.parametrize("H,W", RECT_SIZES)
def test_valid_rect_is_the_golden_rectangle(harness, g, H, W):
    masks = g[f"rect_masks_{H}x{W}"]
    assert masks.shape == (4, H, W) and not masks[2].any() and 0 < masks[1].max() and (masks[1] >= 1).sum() == 1
    for k in RECT_KS:
        assert np.array_equal(h_rect(harness, masks, k), g[f"rect_{H}x{W}_k{k}"]), (H, W, k)
    # two sides of the corner blob clip and two do not (k = 5 on 20 x 24: x, y at 0; the far sides inside the image)
    x, y, w, h = g["rect_20x24_k5"][0]
    assert (x, y) == (0, 0) and w < 24 and h < 20


def test_valid_mask_of_the_reference_datum(harness, g):
    for kind in KINDS:
        rect = h_rect(harness, g[f"{kind}_in_masks"].astype(np.float32), DATUM_K[kind])
        for idx in range(3):
            assert np.array_equal(h_valid(harness, 20, 24, rect[idx]), g[f"{kind}_test_{idx}_valid_mask"]), (kind, idx)
        for idx in range(2):
            full = h_valid(harness, 20, 24, rect[idx])
            want = g[f"{kind}_train_{idx}_valid_mask"]
            assert want.shape == (10, 1) and want.dtype == bool         # the sampler hands every extra array back as [n, -1]
            assert np.array_equal(full[g[f"{kind}_train_{idx}_pixel_indices"]], want[:, 0]), (kind, idx)


def test_downscale_rules_against_numpy(harness, g):
    for s in (2, 4):
        for tag in ("u8", "f32"):
            x = g[f"down_src_{tag}"]
            lo = s // 2 - 1
            a, b, c, d = x[:, lo::s, lo::s], x[:, lo::s, lo + 1::s], x[:, lo + 1::s, lo::s], x[:, lo + 1::s, lo + 1::s]
            want = ((a.astype(np.int32) + b + c + d + 2) >> 2).astype(np.uint8) if tag == "u8" else ((a + b) + (c + d)) * np.float32(0.25)
            got = h_down(harness, x, s)
            assert got.dtype == want.dtype and np.array_equal(bits(got), bits(want)), (s, tag)
            assert np.array_equal(bits(got), bits(g[f"down_{tag}_s{s}"])), (s, tag)
    # the f32 rule is exact on multiples of 1/4: the mean of the four in any order
    q = g["down_src_f32"][:1]
    assert np.array_equal(q * 4, np.round(q * 4))
    assert np.array_equal(h_down(harness, q, 2), q.reshape(1, 20, 2, 24, 2).astype(np.float64).mean((2, 4)).astype(np.float32))
    # the downscaled frames of the fixture: what the reference's __getitem__ made of the 40 x 48 files
    table = (np.arange(256) / 255).astype(np.float32)
    for kind in KINDS:
        sel = g[f"{kind}_ds2_in_images"][::2]
        assert np.array_equal(bits(table[h_down(harness, sel, 2)].reshape(2, -1, 3)),
                              bits(np.stack([g[f"{kind}_ds2_{i}_rgb"] for i in range(2)]))), kind
        m = g[f"{kind}_ds2_in_masks"][::2]
        small = h_down(harness, m, 2).astype(np.float32) if m.dtype == np.uint8 else h_down(harness, m.astype(np.float32), 2)
        assert np.array_equal(bits(small.reshape(2, -1)), bits(np.stack([g[f"{kind}_ds2_{i}_alpha"] for i in range(2)]))), kind


def test_rays_d_of_the_host_replay_is_the_recorded_bar(harness, g):
    from intrinsicavatar_amd import data
    worst = 0.0
    for tag, pre in (("rana", "rana_test_0"), ("synthetichuman", "synthetichuman_test_0"), ("rana_ds2", "rana_ds2_0"),
                     ("synthetichuman_ds2", "synthetichuman_ds2_0")):
        K = g[f"{tag}_in_K"].astype(np.float32)
        if tag.endswith("ds2"):
            K[:2] /= 2
        c2w = np.linalg.inv(g[f"{tag}_in_RT"].astype(np.float32))
        o, d = np.zeros((480, 3), np.float32), np.zeros((480, 3), np.float32)
        harness.truth_h_rays(C.c_int64(480), C.c_int(24), data.camera_words(K, c2w), vp(o), vp(d))
        assert np.array_equal(bits(o), bits(g[f"{pre}_rays_o"])), tag
        err = float(np.abs(d.astype(np.float64) - g[f"{pre}_rays_d"]).max())
        print(f"{tag}: rays_d host replay against the reference's float32 make_rays, max abs {err:.3e}")
        worst = max(worst, err)
    recorded = json.load(open(BARS))["rays_d_host_max_abs"]
    assert worst == recorded, (worst, recorded)
    assert 0 < dir_bound() <= 1e-6 and dir_bound() == min(4 * recorded, 1e-6)


def _host(data, roots, kind, tag, **kw):
    return data.truth_host(kind, roots[tag], "subject", **kw)


@pytest.mark.parametrize("kind", KINDS)
def test_truth_host_against_the_reference(g, roots, kind):
    from intrinsicavatar_amd import data
    cases = (("train", kind, f"{kind}_train", dict(split="train", start=0, end=2, skip=1, downscale=1)),
             ("test", kind, f"{kind}_test", dict(split="test", start=0, end=2, skip=1, downscale=1, near=1.25, far=4.5)),
             ("ds2", f"{kind}_ds2", f"{kind}_ds2", dict(split="train", start=0, end=2, skip=2, downscale=2)))
    for name, tag, pre, kw in cases:
        h = _host(data, roots, kind, tag, **kw)
        base = lambda paths: [os.path.basename(p) for p in paths]      # noqa: E731
        for key, rec in (("img_lists", "img"), ("albedo_lists", "albedo"), ("normal_lists", "normal"), ("msk_lists", "msk")):
            assert base(h[key]) == g[f"{pre}_host_{rec}"].tolist(), (name, key)
        assert os.path.basename(os.path.dirname(h["img_lists"][0])) == str(g[f"{pre}_host_img_dir"])
        if kind == "synthetichuman":
            assert ("images_relit/00" if name == "test" else "images/00") in h["img_lists"][0]
        for k in ("betas", "body_pose", "global_orient", "transl"):
            want = g[f"{pre}_host_{k}"]
            assert h[k].dtype == np.float32 and h[k].shape == want.shape and np.array_equal(bits(h[k]), bits(want)), (name, k)
        assert h["w2c"].dtype == np.float32 and np.array_equal(bits(h["w2c"]), bits(g[f"{pre}_host_w2c"]))
        assert h["c2w"].dtype == np.float32 and np.array_equal(bits(h["c2w"]), bits(np.linalg.inv(g[f"{pre}_host_w2c"])))
        K = g[f"{tag}_in_K"].astype(np.float32)
        if name == "ds2":
            K[:2] /= 2
        assert h["K"].dtype == np.float32 and np.array_equal(bits(h["K"]), bits(K))
        assert h["img_wh"] == tuple(int(v) for v in g[f"{pre}_host_img_wh"]) == (h["width"], h["height"])
        assert h["dilate_k"] == {"rana": 100, "synthetichuman": 50}[kind] and h["downscale"] == kw["downscale"]
        frames = range(2) if name in ("train", "ds2") else range(3)
        prefix = {"train": f"{kind}_train", "test": f"{kind}_test", "ds2": f"{kind}_ds2"}[name]
        for idx in frames:
            for k in ("near", "far"):
                want = g[f"{prefix}_{idx}_{k}"]
                assert want.dtype == np.float32 and len(np.unique(want)) == 1
                assert h[k].dtype == np.float32 and bits(h[k][idx:idx + 1])[0] == bits(want[:1])[0], (name, idx, k)
        if name == "test":
            assert base(h["hdri_files"]) == g[f"{pre}_host_hdri"].tolist() == ["a.hdr", "b.hdr", "a.hdr"]
            assert all(os.path.dirname(p) == os.path.join(roots[tag], "hdri") for p in h["hdri_files"])
        else:
            assert h["hdri_files"] is None
    with pytest.raises(ValueError):
        data.truth_host("zju", roots[kind], "subject", "train", 0, 2)


@pytest.mark.parametrize("kind", KINDS)
def test_odd_or_non_dividing_downscale_raises(roots, kind):
    from intrinsicavatar_amd import data
    for ds in (3, 1.5, 6, 16, 0):                      # odd; fractional; even but 20 % 6 != 0; 24 % 16 != 0; nonsense
        with pytest.raises(NotImplementedError, match="downscale"):
            data.truth_host(kind, roots[kind], "subject", "train", 0, 2, downscale=ds)
    assert data.truth_host(kind, roots[kind], "subject", "train", 0, 2, downscale=4)["img_wh"] == (6, 5)
    assert data.truth_host(kind, roots[kind], "subject", "train", 0, 2, downscale=2.0)["downscale"] == 2


def test_new_entry_points_are_declared_and_exported():
    from intrinsicavatar_amd import _lib, build
    protos = _lib.header_prototypes()
    new = ("ia_truth_valid_rect", "ia_sample_truth", "ia_downscale_center_u8", "ia_downscale_center_f32")
    assert all(n in protos for n in new)
    so = C.CDLL(build.build())
    assert all(hasattr(so, n) for n in new)
    assert len(protos["ia_sample_truth"][1]) == 13 and len(protos["ia_truth_valid_rect"][1]) == 7


def test_cpu_tensors_and_peoplesnapshot_downscale_keep_raising(roots, tmp_path):
    import torch
    from intrinsicavatar_amd import _lib, data
    with pytest.raises(_lib.IaError):
        data.TruthFrames.from_rana(roots["rana"], "subject", "train", 0, 2, device="cpu")
    with pytest.raises(_lib.IaError):
        data.valid_rect(torch.zeros((1, 4, 4)), 5)
    with pytest.raises(_lib.IaError):
        data.downscale_center(torch.zeros((1, 4, 4)), 2)
    with pytest.raises(NotImplementedError, match="downscale"):
        data.TrainingFrames.from_peoplesnapshot(str(tmp_path), "train", 0, 2, downscale=2)
    with pytest.raises(NotImplementedError, match="downscale"):
        data.TruthFrames.from_peoplesnapshot(str(tmp_path), "train", 0, 2, downscale=2)
