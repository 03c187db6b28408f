"""Ground-truth frames on the MI355X (csrc/data.hip: ia_truth_valid_rect, ia_sample_truth, ia_downscale_center_*; data.TruthFrames;
system.evaluate_sequence) against tests/golden/golden_truth.npz: the reference's own RANADataset / SyntheticHumanDataset.__getitem__, run by
tests/golden/make_golden_truth.py with cv2 stubbed by the documented formulas and np.random.randint replayed from recorded words.

Everything is bit for bit, dtypes and shapes as the DataLoader collates them at batch size 1, except the ray directions: the reference
forms them in float32, the kernel in fp64 with one rounding.  Their bound is 4 x the difference of the host replay measured on this fixture
(tests/golden/truth_parity_bars.json, checked by tests/test_truth_cpu.py; the margin is for the summation order of the reference's BLAS)
and never above 1e-6."""
import os

import numpy as np
import pytest
import torch

from tests.test_truth_cpu import DATUM_K, KINDS, RECT_KS, RECT_SIZES, collated, dir_bound, load_golden, write_dataset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLER = {"_target_": "utils.sampler.EdgeSampler", "num_sample": 10, "ratio_mask": 0.6, "ratio_edge": 0.3, "kernel_size": 5}
TRAIN_KEYS = ("rgb", "albedo", "normal", "rays_o", "rays_d", "betas", "global_orient", "body_pose", "transl", "alpha", "valid_mask", "index",
              "t_idx", "w2c", "near", "far")


@pytest.fixture(scope="module")
def g():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from intrinsicavatar_amd import build
    build.build()
    return load_golden()


@pytest.fixture(scope="module")
def roots(g, tmp_path_factory):
    base = tmp_path_factory.mktemp("truth_sets")
    return {tag: write_dataset(str(base / tag), g, tag.split("_")[0], tag) for kind in KINDS for tag in (kind, f"{kind}_ds2")}


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


def compare_datum(b, g, prefix, keys, bound):
    assert sorted(set(b) - {"pixel_indices", "status"}) == sorted(keys)
    for k in keys:
        want = collated(g[f"{prefix}_{k}"])
        if k == "rays_d":
            got = N(b[k])
            assert got.dtype == want.dtype and got.shape == want.shape, k
            err = float(np.abs(got.astype(np.float64) - want).max())
            print(f"{prefix}: rays_d max abs difference {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (prefix, err)
        else:
            assert same(b[k], want), (prefix, k, N(b[k]).dtype, N(b[k]).shape, want.dtype, want.shape)


def train_frames(data, g, roots, kind):
    """the fixture's train split with the dilate kernel its datum was recorded with"""
    host = data.truth_host(kind, roots[kind], "subject", "train", 0, 2, 1)
    host["dilate_k"] = DATUM_K[kind]
    return data.TruthFrames.from_host(host, data.sampler_from_config(SAMPLER), device=DEV), host


@pytest.mark.parametrize("H,W", RECT_SIZES)
def test_valid_rect_is_the_golden_rectangle(g, H, W):
    from intrinsicavatar_amd import data
    masks = T(g[f"rect_masks_{H}x{W}"])                                  # corner blob, fractions + one 1.0 pixel, empty, bottom-right blob
    assert masks.shape == (4, H, W)
    for k in RECT_KS:
        rect = data.valid_rect(masks, k)
        assert same(rect, g[f"rect_{H}x{W}_k{k}"]), (H, W, k, N(rect))
    assert same(data.valid_rect(masks[2:3], 100), np.zeros((1, 4), np.int32))                   # a single, empty frame
    assert same(data.valid_rect(masks[1:2], 1)[:, 2:].contiguous(), np.ones((1, 2), np.int32))  # the 1.0 pixel alone


@pytest.mark.parametrize("kind", KINDS)
def test_batch_is_the_reference_train_datum(g, roots, kind):
    from intrinsicavatar_amd import data
    fr, host = train_frames(data, g, roots, kind)
    assert len(fr) == 3 and fr.img_wh == (24, 20) and fr.valid_dilate == DATUM_K[kind]
    plain = data.TrainingFrames(fr.images, fr.masks, host["K"], host["c2w"], {k: host[k] for k in ("betas", "body_pose", "global_orient", "transl")},
                                fr.sampler)
    plain.near, plain.far = fr.near, fr.far                              # (SyntheticHuman measures from the camera, not from the origin)
    for idx in range(2):
        words = T(g["words"][idx])
        b = fr.batch(idx, words=words)
        fr.check(b)
        assert same(b["pixel_indices"], g[f"{kind}_train_{idx}_pixel_indices"][None])
        compare_datum(b, g, f"{kind}_train_{idx}", TRAIN_KEYS, dir_bound())
        assert b["valid_mask"].dtype == torch.bool and tuple(b["valid_mask"].shape) == (1, 10, 1)
        # the keys shared with TrainingFrames.batch come from the same, unchanged kernel
        p = plain.batch(idx, words=words)
        assert sorted(set(b) - set(p)) == ["albedo", "normal", "valid_mask", "w2c"]
        for k in p:
            assert torch.equal(p[k], b[k]), k
        # a sampled row's truth IS the frame's truth at its pixel
        full = fr.full_frame(idx)
        pix = b["pixel_indices"][0]
        assert torch.equal(full["albedo"][0][pix], b["albedo"][0]) and torch.equal(full["normal"][0][pix], b["normal"][0])
        assert torch.equal(full["valid_mask"][0][pix], b["valid_mask"][0, :, 0])


def test_empty_mask_frame_gives_status_and_zero_truth(g, roots):
    from intrinsicavatar_amd import data
    fr, _ = train_frames(data, g, roots, "rana")
    b = fr.batch(2, words=T(g["words"][0]))                             # frame 2: the empty mask
    assert int(b["status"]) == 3
    with pytest.raises(ValueError):
        fr.check(b)
    nm, ne = fr.sampler.num_mask, fr.sampler.num_edge
    assert bool((b["pixel_indices"][0, :nm + ne] == -1).all()) and bool((b["pixel_indices"][0, nm + ne:] >= 0).all())
    for k in ("albedo", "normal"):
        assert float(b[k][0, :nm + ne].abs().max()) == 0.0, k
        assert float(b[k][0, nm + ne:].abs().max()) > 0.0, k            # the uniform rows still read their pixels
    assert not bool(b["valid_mask"].any()) and same(fr.valid_rect[2], np.zeros(4, np.int32))
    # out-of-range indices, straight at the entry point: zeros and False, nothing read
    from intrinsicavatar_amd import _lib as L
    pix = torch.tensor([0, -1, 20 * 24, 20 * 24 - 1, -7, 2 ** 40], dtype=torch.int64, device=DEV)
    albedo, normal = torch.full((6, 3), 9.0, device=DEV), torch.full((6, 3), 9.0, device=DEV)
    valid = torch.ones(6, dtype=torch.bool, device=DEV)
    L.check(L.lib().ia_sample_truth(L.i64(6), L.i64(0), L.i64(3), L.i32(20), L.i32(24), L.ptr(pix), L.ptr(fr.albedos), L.ptr(fr.normals),
                                    L.ptr(fr.valid_rect), L.ptr(albedo), L.ptr(normal), L.ptr(valid), L.stream()), "ia_sample_truth")
    inside = torch.tensor([True, False, False, True, False, False], device=DEV)
    assert float(albedo[~inside].abs().max()) == 0.0 and float(normal[~inside].abs().max()) == 0.0 and not bool(valid[~inside].any())
    full = fr.full_frame(0)
    assert torch.equal(albedo[inside], full["albedo"][0][[0, 479]]) and torch.equal(valid[inside], full["valid_mask"][0][[0, 479]])


@pytest.mark.parametrize("kind", KINDS)
def test_full_frame_is_the_reference_test_datum(g, roots, kind):
    from intrinsicavatar_amd import data
    host = data.truth_host(kind, roots[kind], "subject", "test", 0, 2, 1, near=1.25, far=4.5)
    host["dilate_k"] = DATUM_K[kind]
    fr = data.TruthFrames.from_host(host, near=1.25, far=4.5, device=DEV)
    assert len(fr) == 3
    seen = []
    for idx in range(3):
        b = fr.full_frame(idx)
        assert int(b["status"]) == 0 and same(b["pixel_indices"], np.arange(480, dtype=np.int64)[None])
        compare_datum(b, g, f"{kind}_test_{idx}", TRAIN_KEYS + ("hdri",), dir_bound())
        assert tuple(b["valid_mask"].shape) == (1, 480) and tuple(b["hdri"].shape) == (1, 4, 8, 3)
        seen.append(b["hdri"])
    assert not bool(fr.full_frame(2)["valid_mask"].any())               # the empty mask: no valid pixel
    assert seen[0].data_ptr() == seen[2].data_ptr() != seen[1].data_ptr(), "frames that name one file share one tensor"
    assert len(fr._hdri) == 2 and fr.HDRI_RESIDENT == 2
    third = os.path.join(roots[kind], "hdri", "c.hdr")
    with open(third, "wb") as f:
        f.write(g["hdr_b"].tobytes())
    assert torch.equal(fr.hdri(third), seen[1]) and len(fr._hdri) == 2, "at most two maps stay resident"
    with pytest.raises(NotImplementedError):
        fr.hdri(os.path.join(roots[kind], "hdri", "light.exr"))
    with pytest.raises(ValueError):
        fr.batch(0)                                                     # no sampler


def test_downscale_kernels(g):
    from intrinsicavatar_amd import data
    for s in (2, 4):
        assert same(data.downscale_center(T(g["down_src_u8"]), s), g[f"down_u8_s{s}"]), s                     # [2,40,48,3] u8
        assert same(data.downscale_center(T(g["down_src_f32"]), s), g[f"down_f32_s{s}"]), s                   # [2,40,48] f32
        one = np.ascontiguousarray(g["down_src_u8"][..., 1])                                                      # [2,40,48] u8: C = 1
        assert same(data.downscale_center(T(one), s), np.ascontiguousarray(g[f"down_u8_s{s}"][..., 1])), s
    for bad in (3, 6, 16):
        with pytest.raises(NotImplementedError, match="downscale"):
            data.downscale_center(T(g["down_src_f32"]), bad)


@pytest.mark.parametrize("kind", KINDS)
def test_downscaled_dataset_is_the_reference_datum(g, roots, kind):
    """downscale = 2 on the 40 x 48 source with the datasets' real dilate kernels; RANA's masks are float64 files, SyntheticHuman's uint8"""
    from intrinsicavatar_amd import data
    make = data.TruthFrames.from_rana if kind == "rana" else data.TruthFrames.from_synthetichuman
    fr = make(roots[f"{kind}_ds2"], "subject", "train", 0, 2, 2, downscale=2, device=DEV)
    assert len(fr) == 2 and (fr.H, fr.W) == (20, 24) and fr.img_wh == (24, 20) and fr.valid_dilate == {"rana": 100, "synthetichuman": 50}[kind]
    for idx in range(2):
        compare_datum(fr.full_frame(idx), g, f"{kind}_ds2_{idx}", TRAIN_KEYS, dir_bound())
    with pytest.raises(NotImplementedError, match="downscale"):
        make(roots[f"{kind}_ds2"], "subject", "train", 0, 2, 2, downscale=3, device=DEV)


def test_batch_does_not_synchronise_and_is_deterministic(g, roots):
    from intrinsicavatar_amd import data
    host = data.truth_host("rana", roots["rana"], "subject", "train", 0, 2, 1)
    host["dilate_k"] = 5
    fr = data.TruthFrames.from_host(host, data.EdgeSampler(300, kernel_size=5), device=DEV)      # more than one workgroup of rows
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
    assert int(idx.min()) >= 0 and int(idx.max()) < 480 and idx.unique().numel() > 100
    full = fr.full_frame(0)
    assert torch.equal(full["albedo"][0][idx], a["albedo"][0]) and torch.equal(full["valid_mask"][0][idx], a["valid_mask"][0, :, 0])
    assert bool(a["valid_mask"].any()) and not bool(a["valid_mask"].all())


def test_evaluate_sequence(g, tmp_path, monkeypatch):
    """two frames of 16 x 16 of the synthetic model at spp 16, each lit by its own HDRI: every frame's metrics and model outputs equal a
    hand-made prepare_frame -> preprocess_data -> evaluate_frame with the same random tensors, mean_metrics is the mean over the frames, and
    the emitter is rebuilt only when the HDRI changes."""
    from intrinsicavatar_amd import animation, data, fields, io_formats, metrics as M, pbr, smpl, system, synthetic as S
    GA = np.load(os.path.join(HERE, "golden", "golden_animation.npz"))
    np.savez(str(tmp_path / "cameras.npz"), intrinsic=np.eye(3), extrinsic=np.eye(4), height=np.int64(1080), width=np.int64(1080))
    np.savez(str(tmp_path / "poses.npz"), poses=GA["aist_in_poses"], trans=GA["aist_in_trans"])
    host = data.animation_host(str(tmp_path), np.zeros(10), start=0, end=4, skip=4, downscale=67.5)
    assert (host["height"], host["width"]) == (16, 16) and len(host["transl"]) == 2
    rng = np.random.default_rng(3)
    hdri_files = []
    for name in ("a", "b"):
        hdri_files.append(str(tmp_path / f"{name}.hdr"))
        io_formats.save_hdr(hdri_files[-1], (rng.random((8, 16, 3)) * 30).astype(np.float32))
    y, x = np.mgrid[0:16, 0:16]
    body_mask = (((x - 7.5) / 4.6) ** 2 + ((y - 8) / 6.6) ** 2 <= 1).astype(np.float32)                     # 9 wide, 13 high
    masks = np.stack([body_mask, np.roll(body_mask, 1, axis=1)])
    u8 = lambda: T(rng.integers(0, 256, (2, 16, 16, 3), dtype=np.uint8))      # noqa: E731
    frames = data.TruthFrames(u8(), T(masks), host["K"], np.linalg.inv(host["w2c"][0]), {k: host[k] for k in ("betas", "body_pose", "global_orient", "transl")},
                              albedos=u8(), normals=u8(), w2c=host["w2c"][0], valid_dilate=3, hdri_files=hdri_files,
                              near_far=(host["near"], host["far"]))
    rects = N(frames.valid_rect)
    ys, xs = np.nonzero(body_mask)
    assert rects[0].tolist() == [xs.min() - 1, ys.min() - 1, xs.max() - xs.min() + 3, ys.max() - ys.min() + 3]      # k = 3: one pixel each side
    assert rects[:, 2:].min() >= 7 and np.ptp(xs) + 1 >= 7 and np.ptp(ys) + 1 >= 7 and frames.img_wh == (16, 16)    # SSIM is defined
    rs, _, _ = S.build_frame(DEV, 16, 16, pose_seed=0, beta=0.01, num_samples_per_ray=64, grid_D=16, grid_H=64, grid_W=64, smooth_iters=5,
                             hash_amp=2e-3)
    mat = fields.VolumeMaterial(seed=2).to(DEV)
    eye = torch.eye(24, device=DEV)
    body = smpl.SMPLKinematics(torch.from_numpy(S.JOINTS).to(DEV), torch.zeros((24, 3, 10), device=DEV), torch.zeros((207, 72), device=DEV),
                               eye, S.PARENTS.tolist(), eye)
    kw = dict(cano_pose=(0.0, 0.0, 0.0, 0.0), occ_res=32)
    built = []
    inner = pbr.EnvironmentLightTensor.update_pdf
    monkeypatch.setattr(pbr.EnvironmentLightTensor, "update_pdf", lambda self, *a, **k: (built.append(1), inner(self, *a, **k))[1])
    dt = body.v_template.dtype
    rest = body.forward(frames.betas[:1].to(dt), smpl.rest_pose(kw["cano_pose"], device=DEV).to(dt), torch.zeros((1, 3), dtype=dt, device=DEV))
    A_rest_inv = torch.linalg.inv(rest["A"].float())

    gen, gen2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    rebuilt, per_frame = [], []
    seq = system.evaluate_sequence(rs, mat, frames, body, 16, generator=gen, **kw)
    for want_idx in range(2):
        before = len(built)
        idx, ret, out = next(seq)
        rebuilt.append(len(built) - before)
        assert idx == want_idx and sorted(ret) == sorted(system.METRIC_KEYS)
        # ---- by hand, with the same draws in the same order
        occ_rand = animation._rand((32 ** 3, 3, 3), DEV, gen2)
        light_u = animation._rand((16, 3), DEV, gen2)
        shuffle_u = animation._rand((256, 16), DEV, gen2)
        assert torch.equal(light_u, out["light_u"]) and torch.equal(shuffle_u, out["shuffle_u"])
        batch = dict(frames.full_frame(idx))
        batch.pop("pixel_indices"), batch.pop("status")
        animation.prepare_frame(rs, body, A_rest_inv, batch, occ_rand, 32)
        batch, bg, _ = system.preprocess_data(batch, "test")
        env = pbr.EnvironmentLightTensor(batch["hdri"].contiguous())
        env.update_pdf()
        hand, hand_out = system.evaluate_frame(rs, batch, mat, env, 16, light_u, shuffle_u, img_wh=(16, 16), stage="test", background_color=bg,
                                               global_illumination=True, render_mode="light")
        for k in hand:
            assert N(ret[k]).tobytes() == N(hand[k]).tobytes(), (idx, k)
        for k, v in hand_out.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(v, out[k]), (idx, k)
        assert "aligned_albedo" in out and tuple(out["comp_rgb_phys_full"].shape) == (256, 3)
        per_frame.append(ret)
    with pytest.raises(StopIteration):
        next(seq)
    assert rebuilt == [1, 1]                                            # two files: one emitter each
    host_vals = [M.to_host(m) for m in per_frame]
    mean = system.mean_metrics(per_frame)
    assert sorted(mean) == sorted(system.METRIC_KEYS)
    for k in mean:
        assert np.isfinite(mean[k]) and mean[k] == float(np.mean([h[k] for h in host_vals])), k
    # the same file twice: ONE emitter; resample_light=False: ONE light_u
    before = len(built)
    lights = [out["light_u"] for _, _, out in system.evaluate_sequence(rs, mat, frames, body, 16, generator=gen, frames_idx=(0, 0),
                                                                        resample_light=False, **kw)]
    assert len(built) - before == 1 and len(lights) == 2 and torch.equal(lights[0], lights[1])
    # an emitter that was passed in is used as it is
    before = len(built)
    env = pbr.EnvironmentLightTensor(frames.hdri(hdri_files[0])[0].contiguous())
    env.update_pdf()
    assert len(list(system.evaluate_sequence(rs, mat, frames, body, 16, emitter=env, generator=gen, frames_idx=(1,), **kw))) == 1
    assert len(built) - before == 1
