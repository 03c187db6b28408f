"""Training batches without a GPU: intrinsicavatar_amd/csrc/data_math.h replayed on the host by tests/data_harness.c against
tests/golden/golden_data.npz (the reference's own make_rays / EdgeSampler.sample / UniformSampler.sample with cv2 stubbed by the
documented formula and np.random.randint replayed from recorded words, tests/golden/make_golden_data.py), plus the samplers' arguments.

Everything is bit for bit except the ray directions: both sides round an fp64 result to float32 and the fp64 values differ only in
summation order (numpy's matmul against the header's left-to-right sums), so one float32 ulp at 1.0 -- 1.2e-7 absolute -- is the bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "golden_data.npz")
DIR_BOUND = 1.2e-7
WINDOW_LENGTHS = (1, 7, 255, 256, 257, 1961)
WINDOW_KS = (1, 5, 16, 32, 64)

vp = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731


def build_harness(directory):
    so = os.path.join(str(directory), "libdata_harness.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-fvisibility=hidden", "-o", so,
                           os.path.join(HERE, "data_harness.c"), "-lm"])
    return C.CDLL(so)


def load_golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("data"))


@pytest.fixture(scope="module")
def g():
    return load_golden()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def h_window(h, x, k, axis=-1):
    x = np.ascontiguousarray(x, np.float32)
    axis %= x.ndim
    outer, inner = int(np.prod(x.shape[:axis], dtype=np.int64)), int(np.prod(x.shape[axis + 1:], dtype=np.int64))
    lo, hi = np.zeros_like(x), np.zeros_like(x)
    h.data_h_window(C.c_int64(outer), C.c_int64(x.shape[axis]), C.c_int64(inner), C.c_int(k), vp(x), vp(lo), vp(hi))
    return lo, hi


def h_pick(h, words, n):
    words = np.ascontiguousarray(words, np.int64)
    out = np.zeros_like(words)
    h.data_h_pick(C.c_int64(words.size), vp(words), C.c_int64(n), vp(out))
    return out


def h_rays(h, K, c2w, W, pixels):
    from intrinsicavatar_amd import data
    pixels = np.ascontiguousarray(pixels, np.int64)
    o, d = np.zeros((pixels.size, 3), np.float32), np.zeros((pixels.size, 3), np.float32)
    h.data_h_rays(C.c_int64(pixels.size), vp(pixels), C.c_int(W), data.camera_words(K, c2w), vp(o), vp(d))
    return o, d


def edge_lists(h, mask, k):
    flat = np.ascontiguousarray(mask, np.float32).reshape(-1)
    lo, hi = h_window(h, flat, k)
    return np.where(flat)[0], np.where(hi - lo)[0]


@pytest.mark.parametrize("n", WINDOW_LENGTHS)
def test_window_flat_bit_identical(harness, g, n):
    for ki, k in enumerate(WINDOW_KS):
        lo, hi = h_window(harness, g[f"win_in_{n}"], k)                  # [7, n]: one array per row
        assert np.array_equal(bits(lo), bits(g[f"win_min_{n}"][ki])), (n, k)
        assert np.array_equal(bits(hi), bits(g[f"win_max_{n}"][ki])), (n, k)


@pytest.mark.parametrize("tag", ["37x53", "64x64"])
def test_window_two_passes_are_the_square_kernel(harness, g, tag):
    x = g[f"win2d_in_{tag}"]
    for ki, k in enumerate(WINDOW_KS):
        row_lo, row_hi = h_window(harness, x, k, -1)
        lo, hi = h_window(harness, row_lo, k, -2)[0], h_window(harness, row_hi, k, -2)[1]
        assert np.array_equal(bits(lo), bits(g[f"win2d_min_{tag}"][ki])), (tag, k)
        assert np.array_equal(bits(hi), bits(g[f"win2d_max_{tag}"][ki])), (tag, k)


def test_u8_table_and_edge_test(harness, g):
    table = np.zeros(256, np.float32)
    harness.data_h_u8_table(vp(table))
    assert np.array_equal(bits(table), bits((np.arange(256) / 255).astype(np.float32)))
    img = g["big_image"].reshape(-1, 3)
    assert np.array_equal(bits(table[img[g["big_edge_indices"]]]), bits(g["big_edge_rgb"]))
    assert harness.data_h_is_edge(C.c_float(0.25), C.c_float(0.5)) == 1 and harness.data_h_is_edge(C.c_float(0.5), C.c_float(0.5)) == 0


@pytest.mark.parametrize("name,k", [("big_edge", 16), ("big_norand", 16), ("big_uniform", 0), ("small_edge", 5), ("small_norand", 5),
                                    ("small_uniform", 0)])
def test_index_rule_reproduces_the_reference_draws(harness, g, name, k):
    mask = g[name.split("_")[0] + "_mask"]
    n_mask, n_edge, n_rand = (int(v) for v in g[f"{name}_split"])
    words = g[f"{name}_words"]
    parts = []
    if k:
        mask_loc, edge_loc = edge_lists(harness, mask, k)
        assert len(mask_loc) and len(edge_loc)
        parts += [mask_loc[h_pick(harness, words[:n_mask], len(mask_loc))], edge_loc[h_pick(harness, words[n_mask:n_mask + n_edge], len(edge_loc))]]
    parts.append(h_pick(harness, words[n_mask + n_edge:], mask.size))
    idx = np.concatenate(parts)
    assert np.array_equal(idx, g[f"{name}_indices"])
    assert np.array_equal(bits(mask.reshape(-1)[idx]), bits(g[f"{name}_alpha"]))


def test_lists_of_three_frames(harness, g):
    for f in range(3):
        mask_loc, edge_loc = edge_lists(harness, g["lists_masks"][f], 5)
        assert np.array_equal(mask_loc, g[f"lists_mask_loc_{f}"]) and np.array_equal(edge_loc, g[f"lists_edge_loc_{f}"])
    assert len(g["lists_mask_loc_1"]) == 0 and len(g["lists_edge_loc_1"]) == 0


def test_rays_origins_bitwise_directions_within_one_ulp(harness, g):
    differing = {}
    for cam, pixels, W in (("cam0", g["cam0_sel"], 540), ("cam1", np.arange(20 * 24), 24)):
        o, d = h_rays(harness, g[f"{cam}_K"], g[f"{cam}_c2w"], W, pixels)
        want_o, want_d = g[f"{cam}_rays_o"].reshape(-1, 3), g[f"{cam}_rays_d"].reshape(-1, 3)
        assert np.array_equal(bits(o), bits(want_o)), cam
        err = float(np.abs(d.astype(np.float64) - want_d).max())
        differing[cam] = (int((bits(d) != bits(want_d)).sum()), d.size, err)
        assert err <= DIR_BOUND, (cam, err)
        assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 2e-7
    print("direction elements that differ from the reference at all (count, of, max abs):", differing)
    # the sampled rows of the reference are rows of its frame: the same statement through the samplers' outputs
    o, d = h_rays(harness, g["cam0_K"], g["cam0_c2w"], 540, g["big_edge_indices"])
    assert np.array_equal(bits(o), bits(g["big_edge_rays_o"]))
    assert np.abs(d.astype(np.float64) - g["big_edge_rays_d"]).max() <= DIR_BOUND


def test_sampler_arguments():
    from intrinsicavatar_amd import data
    with pytest.raises(AssertionError):
        data.EdgeSampler(4096, ratio_mask=0.8, ratio_edge=0.3)
    with pytest.raises(AssertionError):
        data.EdgeSampler(4096, ratio_mask=-0.1)
    with pytest.raises(AssertionError):
        data.EdgeSampler(4096, ratio_edge=-0.1)
    with pytest.raises(ValueError):
        data.EdgeSampler(4096, kernel_size=65)
    s = data.EdgeSampler(4096)
    assert (s.num_mask, s.num_edge, s.num_rand, s.kernel_size, s.two_dimensional) == (int(4096 * 0.6), int(4096 * 0.3), 4096 - 2457 - 1228, 32, False)
    assert (s.num_mask, s.num_edge, s.num_rand) == (2457, 1228, 411)
    s = data.EdgeSampler(10)
    assert (s.num_mask, s.num_edge, s.num_rand) == (6, 3, 1)
    s = data.EdgeSampler(10, 0.7, 0.3, 5)
    assert (s.num_mask, s.num_edge, s.num_rand) == (7, 3, 0)
    u = data.UniformSampler(4096)
    assert (u.num_mask, u.num_edge, u.num_rand, u.num_sample) == (0, 0, 4096, 4096)
    e = data.sampler_from_config({"_target_": "utils.sampler.EdgeSampler", "num_sample": 4096, "ratio_mask": 0.6, "ratio_edge": 0.3,
                                  "kernel_size": 16})
    assert isinstance(e, data.EdgeSampler) and e.kernel_size == 16
    assert isinstance(data.sampler_from_config({"_target_": "utils.sampler.UniformSampler", "num_sample": 7}), data.UniformSampler)
    for cls in (data.BalancedSampler, data.PatchSampler):
        with pytest.raises(NotImplementedError, match="np.random.choice"):
            cls(16)


def test_fixture_splits_are_the_constructor_splits(g):
    from intrinsicavatar_amd import data
    for name, kw in (("big_edge", dict(num_sample=4096, ratio_mask=0.6, ratio_edge=0.3, kernel_size=16)),
                     ("big_norand", dict(num_sample=4096, ratio_mask=0.75, ratio_edge=0.25, kernel_size=16)),
                     ("small_norand", dict(num_sample=10, ratio_mask=0.7, ratio_edge=0.3, kernel_size=5))):
        s = data.EdgeSampler(**kw)
        assert [s.num_mask, s.num_edge, s.num_rand] == g[f"{name}_split"].tolist()


def test_downscale_and_cpu_tensors_raise(tmp_path):
    from intrinsicavatar_amd import _lib, data
    with pytest.raises(NotImplementedError, match="downscale"):
        data.TrainingFrames.from_peoplesnapshot(str(tmp_path), "train", 0, 2, downscale=2)
    with pytest.raises(_lib.IaError):
        data.TrainingFrames.from_peoplesnapshot(str(tmp_path), "train", 0, 2, device="cpu")
    with pytest.raises(_lib.IaError):
        data.make_rays(np.eye(3), np.eye(4), 4, 4, "cpu")
    with pytest.raises(_lib.IaError):
        data.EdgeSampler(16, kernel_size=5).edge_band(torch.zeros((4, 4)))
    smpl = dict(betas=np.zeros(10), body_pose=np.zeros((1, 69)), global_orient=np.zeros((1, 3)), transl=np.zeros((1, 3)))
    with pytest.raises(_lib.IaError):
        data.TrainingFrames(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), torch.zeros((1, 4, 4)), np.eye(3), np.eye(4), smpl,
                            data.UniformSampler(4))
