"""CPU: bench.py's --dump-outputs writer (bench.dump_outputs) on host tensors -- per-ray maps in ray order over the chunks, one loss
per chunk, parameters and gradients by position, fixed samples of large frames and tensors, the same files from run to run."""
import os

import numpy as np
import torch


def _bench():
    env = dict(os.environ)
    try:
        import bench                # sets thread-count defaults in os.environ for its own process: keep this one's as they were
    finally:
        os.environ.clear()
        os.environ.update(env)
    return bench


def _outs(n_chunk, chunks, seed):
    g = torch.Generator().manual_seed(seed)
    ch = {"opacity": 1, "roughness": 1, "metallic": 1}
    return [dict({k: torch.rand((n_chunk, ch.get(k, 3)), generator=g) for k in _bench().DUMP_RAY_MAPS}, loss=torch.rand((), generator=g))
            for _ in range(chunks)]


def test_dump_outputs_writes_the_step_in_ray_order(tmp_path):
    B = _bench()
    outs = _outs(100, 3, 0)
    small, big = torch.nn.Parameter(torch.rand(7, 5)), torch.nn.Parameter(torch.rand(B.DUMP_MAX_ENTRIES + 1000))
    small.grad, big.grad = torch.rand(7, 5), None
    B.dump_outputs(str(tmp_path), outs, [small, big])
    got = {f.stem: np.load(f) for f in tmp_path.glob("*.npy")}
    assert np.array_equal(got["comp_rgb"], torch.cat([o["comp_rgb"] for o in outs]).numpy())
    assert got["opacity"].shape == (300, 1) and "ray_index" not in got
    assert np.array_equal(got["loss"], np.array([float(o["loss"]) for o in outs], np.float32))
    assert np.array_equal(got["param_000"], small.detach().reshape(-1).numpy()) and np.array_equal(got["grad_000"], small.grad.reshape(-1).numpy())
    assert got["param_001"].shape == (B.DUMP_MAX_ENTRIES,) and "grad_001" not in got
    assert np.isin(got["param_001"], big.detach().numpy()).all()
    assert all(a.dtype == np.float32 for a in got.values())


def test_dump_outputs_samples_large_frames_the_same_way_every_run(tmp_path):
    B = _bench()
    n = B.DUMP_MAX_RAYS + 4096
    outs = _outs(n // 2, 2, 1)
    p = torch.nn.Parameter(torch.rand(3 * B.DUMP_MAX_ENTRIES))
    p.grad = torch.rand(3 * B.DUMP_MAX_ENTRIES)
    B.dump_outputs(str(tmp_path / "a"), outs, [p])
    B.dump_outputs(str(tmp_path / "b"), outs, [p])
    a = {f.stem: np.load(f) for f in (tmp_path / "a").glob("*.npy")}
    b = {f.stem: np.load(f) for f in (tmp_path / "b").glob("*.npy")}
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["ray_index"].astype(np.int64)
    assert a["ray_index"].dtype == np.float64 and len(np.unique(idx)) == B.DUMP_MAX_RAYS and idx.max() < n
    assert np.array_equal(a["comp_rgb_phys"], torch.cat([o["comp_rgb_phys"] for o in outs]).numpy()[idx])
    assert sum(x.nbytes for x in a.values()) <= B.DUMP_MAX_BYTES
