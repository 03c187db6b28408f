"""Time a training batch built on the device (TrainingFrames.batch: torch.randint + one kernel) and the construction of the resident
dataset (edge band + index lists of every frame), next to the same batch written with torch operators on the device (max_pool1d for the
band and nonzero per frame at construction; randint, remainder, indexing per step) -- the only baseline: the package had no such path
before.  Device-timed (events), warm-up, medians over repeats; the numbers are reported, nothing is asserted on them.

    python tools/data_batch_bench.py [--frames 112] [--size 1080] [--rays 4096] [--repeats 30] [--out profiles/data_batch.json]
"""
import argparse
import json
import os
import statistics
import sys

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402


def timed(fn, repeats, warmup=3):
    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), out


def synthetic_frames(F, S, dev):
    """a moving ellipse per frame (about a fifth of the pixels) and a patterned image, generated on the device"""
    y, x = torch.meshgrid(torch.arange(S, device=dev), torch.arange(S, device=dev), indexing="ij")
    masks = torch.empty((F, S, S), dtype=torch.float32, device=dev)
    images = torch.empty((F, S, S, 3), dtype=torch.uint8, device=dev)
    for f in range(F):
        cx, cy = S * (0.45 + 0.1 * np.sin(0.3 * f)), S * 0.52
        masks[f] = ((((x - cx) / (0.17 * S)) ** 2 + ((y - cy) / (0.4 * S)) ** 2) <= 1).float()
        images[f] = torch.stack([(x * 3 + y * 5 + f) % 256, (x * 7 + y * 2 + 40 * f) % 256, (x + y * y + f) % 256], -1).to(torch.uint8)
    return images, masks


class TorchFrames:
    """the same batch through torch operators on resident frames"""

    def __init__(self, images, masks, K, c2w, k, split, near, far):
        F, S = masks.shape[0], masks.shape[1]
        self.images, self.masks, self.N, self.split, self.near, self.far = images.view(F, -1, 3), masks.view(F, -1), S * S, split, near, far
        flat = self.masks[:, None, :]
        pad = (k // 2, k - 1 - k // 2)
        mask_o = Fn.max_pool1d(Fn.pad(flat, pad, value=float("-inf")), k, 1)[:, 0]
        mask_i = -Fn.max_pool1d(Fn.pad(-flat, pad, value=float("-inf")), k, 1)[:, 0]
        self.mask_loc = [self.masks[f].nonzero()[:, 0] for f in range(F)]
        self.edge_loc = [(mask_o[f] - mask_i[f]).nonzero()[:, 0] for f in range(F)]
        dev = masks.device
        p = torch.arange(self.N, device=dev)
        xy = torch.stack([p % S, p // S, torch.ones_like(p)], -1).double()
        d = xy @ torch.from_numpy(np.linalg.inv(K)).to(dev).T @ torch.from_numpy(c2w[:3, :3]).to(dev).T
        self.rays_d = (d / d.norm(dim=1, keepdim=True)).float()
        self.rays_o = torch.from_numpy(c2w[:3, 3]).to(dev).float().expand(self.N, 3)

    def batch(self, f):
        nm, ne, nr = self.split
        w = torch.randint(0, 2 ** 63 - 1, (nm + ne + nr,), dtype=torch.int64, device=self.masks.device)
        ml, el = self.mask_loc[f], self.edge_loc[f]
        idx = torch.cat([ml[w[:nm] % ml.shape[0]], el[w[nm:nm + ne] % el.shape[0]], w[nm + ne:] % self.N])
        n = idx.shape[0]
        return {"pixel_indices": idx, "alpha": self.masks[f][idx], "rgb": (self.images[f][idx].double() / 255).float(),
                "rays_o": self.rays_o[idx], "rays_d": self.rays_d[idx],
                "near": torch.full((n,), self.near, device=idx.device), "far": torch.full((n,), self.far, device=idx.device)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=112)
    ap.add_argument("--size", type=int, default=1080)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_batch.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times the MI355X: it does not run without one"
    from intrinsicavatar_amd import build, data
    build.build()
    dev = torch.device("cuda:0")
    F, S, n = a.frames, a.size, a.rays
    K = np.array([[1500.0 * S / 1080, 0, S / 2], [0, 1500.0 * S / 1080, S / 2], [0, 0, 1]])
    c2w = np.eye(4)
    images, masks = synthetic_frames(F, S, dev)
    smpl = dict(betas=np.zeros(10), body_pose=np.zeros((F, 69)), global_orient=np.zeros((F, 3)), transl=np.tile([0.0, 0.2, 2.6], (F, 1)))
    smp = data.EdgeSampler(n, 0.6, 0.3, 16)                            # configs/sampler/edge.yaml
    make = lambda: data.TrainingFrames(images, masks, K, c2w, smpl, smp, near=1.0, far=4.0)      # noqa: E731
    construct_ms, fr = timed(make, 5, warmup=1)
    band_ms, _ = timed(lambda: smp.edge_band(fr.masks), 5, warmup=1)
    frame = F // 2
    batch_ms, b = timed(lambda: fr.batch(frame), a.repeats)
    words = torch.randint(0, 2 ** 63 - 1, (n,), dtype=torch.int64, device=dev)
    kernel_ms, b = timed(lambda: fr.batch(frame, words=words), a.repeats)
    full_ms, _ = timed(lambda: fr.full_frame(frame), a.repeats)
    fr.check(b)

    split = (smp.num_mask, smp.num_edge, smp.num_rand)
    t_construct_ms, tf = timed(lambda: TorchFrames(images, masks, K, c2w, 16, split, 1.0, 4.0), 3, warmup=1)
    t_batch_ms, _ = timed(lambda: tf.batch(frame), a.repeats)
    lists_equal = bool(torch.equal(tf.mask_loc[frame].int(), fr.mask_loc[int(fr.mask_start[frame]):int(fr.mask_start[frame + 1])])
                       and torch.equal(tf.edge_loc[frame].int(), fr.edge_loc[int(fr.edge_start[frame]):int(fr.edge_start[frame + 1])]))
    out_bytes = n * (8 + 4 + 12 + 12 + 12 + 4 + 4)
    res = {"device": torch.cuda.get_device_name(0), "frames": F, "height": S, "width": S, "rays": n, "kernel_size": 16, "split": list(split),
           "repeats": a.repeats, "timing": "device events, median",
           "list_sizes_of_the_timed_frame": [int(v) for v in fr.counts[frame].tolist()],
           "hip": {"batch_ms": batch_ms, "batch_given_words_ms": kernel_ms, "full_frame_ms": full_ms, "constructor_ms": construct_ms,
                   "edge_band_ms": band_ms, "batch_output_bytes": out_bytes},
           "torch": {"batch_ms": t_batch_ms, "constructor_ms": t_construct_ms},
           "agreement": {"lists_of_the_timed_frame_equal": lists_equal},
           "speedup_batch": t_batch_ms / batch_ms, "speedup_constructor": t_construct_ms / construct_ms}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
