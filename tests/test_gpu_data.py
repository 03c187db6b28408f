"""Training batches on the MI355X (csrc/data.hip through intrinsicavatar_amd/data.py) against tests/golden/golden_data.npz: the
reference's own make_rays / EdgeSampler.sample / UniformSampler.sample / PeopleSnapshotDataset.__getitem__, run by
tests/golden/make_golden_data.py with cv2 stubbed by the documented formula and np.random.randint replayed from recorded words.

Integers, mask values, colours and ray origins are bit for bit.  Ray directions: both sides round an fp64 result to float32 and the fp64
values differ only in summation order, so one float32 ulp at 1.0 -- 1.2e-7 absolute -- is the bound (derived, not measured)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
DIR_BOUND = 1.2e-7
WINDOW_LENGTHS = (1, 7, 255, 256, 257, 1961)
WINDOW_KS = (1, 5, 16, 32, 64)
SAMPLER_CASES = {"big_edge": dict(num_sample=4096, ratio_mask=0.6, ratio_edge=0.3, kernel_size=16),
                 "big_norand": dict(num_sample=4096, ratio_mask=0.75, ratio_edge=0.25, kernel_size=16),
                 "big_uniform": dict(num_sample=4096),
                 "small_edge": dict(num_sample=10, ratio_mask=0.6, ratio_edge=0.3, kernel_size=5),
                 "small_norand": dict(num_sample=10, ratio_mask=0.7, ratio_edge=0.3, kernel_size=5),
                 "small_uniform": dict(num_sample=10)}
DATUM_KEYS = ("rgb", "rays_o", "rays_d", "betas", "global_orient", "body_pose", "transl", "alpha", "index", "t_idx", "near", "far")


@pytest.fixture(scope="module")
def g():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from intrinsicavatar_amd import build
    build.build()
    z = np.load(os.path.join(HERE, "golden", "golden_data.npz"))
    return {k: z[k] for k in z.files}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want):
    """bit for bit, dtype and shape included"""
    got = N(got) if isinstance(got, torch.Tensor) else got
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(bits(got), bits(want))


def zero_smpl(F):
    return dict(betas=np.zeros(10), body_pose=np.zeros((F, 69)), global_orient=np.zeros((F, 3)), transl=np.zeros((F, 3)))


def sampler_for(data, kw):
    return data.EdgeSampler(**kw) if "kernel_size" in kw else data.UniformSampler(**kw)


def frames_for(data, g, name):
    tag = name.split("_")[0]
    cam = "cam0" if tag == "big" else "cam1"
    return data.TrainingFrames(T(g[f"{tag}_image"])[None], T(g[f"{tag}_mask"])[None], g[f"{cam}_K"], g[f"{cam}_c2w"], zero_smpl(1),
                               sampler_for(data, SAMPLER_CASES[name]), near=0.5, far=3.0)


@pytest.mark.parametrize("n", WINDOW_LENGTHS)
def test_window_flat_bit_identical(g, n):
    from intrinsicavatar_amd import data
    x = T(g[f"win_in_{n}"])                                            # [7, n]: seven arrays in one launch
    for ki, k in enumerate(WINDOW_KS):
        lo, hi = data.window_minmax(x, k)
        assert same(lo, g[f"win_min_{n}"][ki]) and same(hi, g[f"win_max_{n}"][ki]), (n, k)
        one_lo, one_hi = data.window_minmax(x[4].contiguous(), k)      # and alone, as a 1-D array
        assert same(one_lo, g[f"win_min_{n}"][ki][4]) and same(one_hi, g[f"win_max_{n}"][ki][4]), (n, k)


@pytest.mark.parametrize("tag", ["37x53", "64x64"])
def test_window_two_dimensional_form(g, tag):
    from intrinsicavatar_amd import data
    x = T(g[f"win2d_in_{tag}"])
    for ki, k in enumerate(WINDOW_KS):
        mask_i, mask_o = data.EdgeSampler(16, kernel_size=k, two_dimensional=True).edge_band(x)
        assert same(mask_i, g[f"win2d_min_{tag}"][ki]) and same(mask_o, g[f"win2d_max_{tag}"][ki]), (tag, k)
        both = torch.stack([x, 1 - x])                                  # batched over frames
        bi, bo = data.EdgeSampler(16, kernel_size=k, two_dimensional=True).edge_band(both)
        assert same(bi[0], g[f"win2d_min_{tag}"][ki]) and same(bo[0], g[f"win2d_max_{tag}"][ki]), (tag, k)
        assert same(bo[1], 1 - g[f"win2d_min_{tag}"][ki]), (tag, k)     # max(1 - x) = 1 - min(x), exact on these values


def test_flat_edge_band_wraps_across_rows(g):
    """the default follows the reference as written: one window over the flat index"""
    from intrinsicavatar_amd import data
    x = g["win2d_in_37x53"]
    mask_i, mask_o = data.EdgeSampler(16, kernel_size=5).edge_band(T(x))
    flat_i, flat_o = data.window_minmax(T(x.reshape(-1)), 5)
    assert same(mask_i, N(flat_i).reshape(37, 53)) and same(mask_o, N(flat_o).reshape(37, 53))
    two_i, _ = data.EdgeSampler(16, kernel_size=5, two_dimensional=True).edge_band(T(x))
    assert not torch.equal(two_i, mask_i)


def test_lists_three_frames_one_empty(g):
    from intrinsicavatar_amd import data
    masks = g["lists_masks"]
    F, H, W = masks.shape
    fr = data.TrainingFrames(torch.zeros((F, H, W, 3), dtype=torch.uint8, device=DEV), T(masks), g["cam1_K"], g["cam1_c2w"], zero_smpl(F),
                             data.EdgeSampler(10, kernel_size=5))
    for name, start, loc, col in (("mask", fr.mask_start, fr.mask_loc, 0), ("edge", fr.edge_start, fr.edge_loc, 1)):
        want = [g[f"lists_{name}_loc_{f}"] for f in range(F)]
        offsets = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.int32)
        assert same(start, offsets), name
        assert same(loc, np.concatenate(want).astype(np.int32)), name
        assert same(fr.counts[:, col].contiguous(), np.array([len(w) for w in want], np.int32)), name
    assert int(fr.counts[1].sum()) == 0


@pytest.mark.parametrize("name", list(SAMPLER_CASES))
def test_samplers_reproduce_the_reference_rows(g, name):
    from intrinsicavatar_amd import data
    fr = frames_for(data, g, name)
    assert [fr.sampler.num_mask, fr.sampler.num_edge, fr.sampler.num_rand] == g[f"{name}_split"].tolist()
    b = fr.batch(0, words=T(g[f"{name}_words"]))
    fr.check(b)
    assert same(b["pixel_indices"][0], g[f"{name}_indices"])
    assert same(b["alpha"][0], g[f"{name}_alpha"])
    assert same(b["rgb"][0], g[f"{name}_rgb"])
    assert same(b["rays_o"][0], g[f"{name}_rays_o"])
    err = float(np.abs(N(b["rays_d"][0]).astype(np.float64) - g[f"{name}_rays_d"]).max())
    print(name, "ray direction max abs difference:", err, "elements differing:", int((bits(N(b["rays_d"][0])) != bits(g[f"{name}_rays_d"])).sum()))
    assert err <= DIR_BOUND
    # a sampled row's rays ARE the frame's rays at its pixel (one device function serves both)
    full = fr.full_frame(0)
    idx = b["pixel_indices"][0]
    for k in ("rays_o", "rays_d", "rgb", "alpha"):
        assert torch.equal(full[k][0][idx], b[k][0]), k
    ro, rd = data.make_rays(g["cam0_K" if name.startswith("big") else "cam1_K"], g["cam0_c2w" if name.startswith("big") else "cam1_c2w"],
                            fr.H, fr.W, DEV)
    assert torch.equal(ro.reshape(-1, 3), full["rays_o"][0]) and torch.equal(rd.reshape(-1, 3), full["rays_d"][0])
    assert same(b["near"][0], np.full(fr.sampler.num_sample, 0.5, np.float32)) and same(b["far"][0], np.full(fr.sampler.num_sample, 3.0, np.float32))


def test_make_rays_against_the_reference_frame(g):
    from intrinsicavatar_amd import data
    ro, rd = data.make_rays(g["cam1_K"], g["cam1_c2w"], 20, 24, DEV)
    assert same(ro, g["cam1_rays_o"])
    assert rd.shape == (20, 24, 3) and float(np.abs(N(rd).astype(np.float64) - g["cam1_rays_d"]).max()) <= DIR_BOUND
    ro, rd = data.make_rays(g["cam0_K"], g["cam0_c2w"], 540, 540, DEV)
    sel = T(g["cam0_sel"])
    assert same(ro.reshape(-1, 3)[sel], g["cam0_rays_o"])
    assert float(np.abs(N(rd.reshape(-1, 3)[sel]).astype(np.float64) - g["cam0_rays_d"]).max()) <= DIR_BOUND


def test_empty_lists_set_the_status_word(g):
    from intrinsicavatar_amd import data
    good = g["small_mask"]
    masks = np.stack([np.zeros_like(good), np.ones_like(good), good])
    images = np.stack([g["small_image"]] * 3)
    fr = data.TrainingFrames(T(images), T(masks), g["cam1_K"], g["cam1_c2w"], zero_smpl(3), data.EdgeSampler(10, kernel_size=5), near=0.5, far=3.0)
    words = T(g["small_edge_words"])
    empty, full, ok = fr.batch(0, words=words), fr.batch(1, words=words), fr.batch(2, words=words)
    assert int(empty["status"]) & 1
    with pytest.raises(ValueError):
        fr.check(empty)
    assert int(full["status"]) == 2                                     # an all-one mask has no edge band
    with pytest.raises(ValueError, match="edge"):
        fr.check(full)
    nm, ne = fr.sampler.num_mask, fr.sampler.num_edge
    assert bool((empty["pixel_indices"][0, :nm + ne] == -1).all()) and bool((empty["pixel_indices"][0, nm + ne:] >= 0).all())
    assert bool((full["pixel_indices"][0, nm:nm + ne] == -1).all()) and bool((full["pixel_indices"][0, :nm] >= 0).all())
    for k in ("rgb", "rays_o", "rays_d", "alpha", "near", "far"):
        assert float(full[k][0, nm:nm + ne].abs().max()) == 0.0, k
    fr.check(ok)                                                        # the good frame of the same set is unaffected
    assert int(ok["status"]) == 0
    assert same(ok["pixel_indices"][0], g["small_edge_indices"]) and same(ok["rgb"][0], g["small_edge_rgb"])


def write_dataset(root, g):
    """the three-frame directory of the fixture, written from its arrays"""
    from PIL import Image
    for d in ("images", "masks", "poses"):
        os.makedirs(os.path.join(root, d))
    np.savez(os.path.join(root, "cameras.npz"), intrinsic=g["ds_cam_intrinsic"], extrinsic=g["ds_cam_extrinsic"], height=20, width=24)
    for i in range(3):
        Image.fromarray(g["ds_images"][i]).save(os.path.join(root, "images", f"image_{i:04d}.png"))
        np.save(os.path.join(root, "masks", f"mask_{i:04d}.npy"), g[f"ds_mask{i}"])
    np.savez(os.path.join(root, "poses", "anim_nerf_train.npz"), betas=g["ds_train_betas"], thetas=g["ds_train_thetas"], transl=g["ds_train_transl"])
    np.savez(os.path.join(root, "poses.npz"), betas=g["ds_poses_betas"], body_pose=g["ds_poses_body_pose"],
             global_orient=g["ds_poses_global_orient"], transl=g["ds_poses_transl"])


def collated(v):
    """what the DataLoader's default collate makes of one datum entry at batch_size 1"""
    v = np.asarray(v)
    if v.ndim == 0:
        v = v.astype(np.int64 if v.dtype.kind == "i" else np.float64)
    return v[None]


@pytest.fixture(scope="module")
def dataset_dir(g, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("peoplesnapshot"))
    write_dataset(root, g)
    return root


def compare_datum(b, g, prefix):
    assert sorted(set(b) - {"pixel_indices", "status"}) == sorted(DATUM_KEYS)
    for k in DATUM_KEYS:
        want = collated(g[f"{prefix}_{k}"])
        if k == "rays_d":
            got = N(b[k])
            assert got.dtype == want.dtype and got.shape == want.shape, k
            assert float(np.abs(got.astype(np.float64) - want).max()) <= DIR_BOUND
        else:
            assert same(b[k], want), (prefix, k, N(b[k]).dtype, N(b[k]).shape, want.dtype, want.shape)


@pytest.mark.parametrize("tag,near,far", [("cfg", 1.25, 4.5), ("transl", None, None)])
def test_batch_is_the_reference_datum(g, dataset_dir, tag, near, far):
    from intrinsicavatar_amd import data
    smp = data.sampler_from_config({"_target_": "utils.sampler.EdgeSampler", "num_sample": 10, "ratio_mask": 0.6, "ratio_edge": 0.3,
                                    "kernel_size": 5})
    fr = data.TrainingFrames.from_peoplesnapshot(dataset_dir, "train", 0, 2, 1, sampler=smp, near=near, far=far, device=DEV)
    assert len(fr) == 3 and fr.masks.dtype == torch.float32
    for idx in range(3):
        b = fr.batch(idx, words=T(g["ds_words"][idx]))
        fr.check(b)
        compare_datum(b, g, f"ds_train_{tag}_{idx}")


def test_full_frame_is_the_reference_test_datum(g, dataset_dir):
    from intrinsicavatar_amd import data
    fr = data.TrainingFrames.from_peoplesnapshot(dataset_dir, "test", 0, 2, 2, device=DEV)
    assert len(fr) == 2
    for idx in range(2):
        compare_datum(fr.full_frame(idx), g, f"ds_test_{idx}")
    with pytest.raises(ValueError):
        fr.batch(0)                                                     # no sampler


def test_batch_does_not_synchronise_and_is_deterministic(g):
    from intrinsicavatar_amd import data
    fr = frames_for(data, g, "big_edge")
    gen = torch.Generator(device=DEV)
    fr.batch(0, generator=gen)                                          # first call: library load, code objects
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        gen.manual_seed(7)
        a = fr.batch(0, generator=gen)
        gen.manual_seed(7)
        b = fr.batch(0, generator=gen)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            gen.manual_seed(7)
            c = fr.batch(0, generator=gen)
        torch.cuda.current_stream().wait_stream(side)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    fr.check(a)
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    idx = a["pixel_indices"][0]
    assert int(idx.min()) >= 0 and int(idx.max()) < 540 * 540 and idx.unique().numel() > 3000
    assert bool((a["alpha"][0, :fr.sampler.num_mask] != 0).all())


def test_batch_goes_through_the_model():
    """keys, layout and usable rays: preprocess_data(..., "train") and one forward_train_ on the synthetic model; no value is compared"""
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from intrinsicavatar_amd import build
    build.build()
    from intrinsicavatar_amd import data, fields, pbr, synthetic as S, system
    from tests.test_gpu_relight_oracle import hdri
    H = W = 48
    rs, rays, _ = S.build_frame(DEV, H, W, pose_seed=0, beta=0.01, num_samples_per_ray=64, grid_D=16, grid_H=64, grid_W=64, smooth_iters=5,
                                hash_amp=1e-2)
    K = S.K_1080.copy()
    K[:2] /= 1080.0 / H
    y, x = np.mgrid[0:H, 0:W]
    mask = ((((x - 24) / 9.0) ** 2 + ((y - 24) / 20.0) ** 2) <= 1).astype(np.float32)
    image = np.stack([x * 5, y * 5, x + y], -1).astype(np.uint8)
    n, spp = 256, 16
    fr = data.TrainingFrames(T(image)[None], T(mask)[None], K, np.eye(4), zero_smpl(1), data.EdgeSampler(n, kernel_size=5))
    gen = torch.Generator(device=DEV).manual_seed(1)
    b = fr.batch(0, generator=gen)
    fr.check(b)
    batch, bg, t_idx = system.preprocess_data(b, "train", "white")
    assert batch["rays"].shape == (n, 8) and batch["rgb"].shape == (n, 3) and batch["alpha"].shape == (n,) and float(t_idx) == 0.0
    mat = fields.VolumeMaterial(seed=2).to(DEV)
    env = pbr.EnvironmentLightTensor(torch.from_numpy(hdri()).to(DEV))
    env.update_pdf()
    light_u = torch.rand((n * spp, 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    out = system.model_forward(rs, batch["rays"], mat, env, spp, light_u, None, training=True, background_color=bg, global_illumination=True)
    assert out["comp_rgb"].shape == (n, 3)
    per_ray = [k for k, v in out.items() if isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == n and v.is_floating_point()]
    assert "comp_rgb" in per_ray and len(per_ray) >= 3
    for k in per_ray:
        assert bool(torch.isfinite(out[k]).all()), k
