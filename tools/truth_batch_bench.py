"""Time a training batch with ground truth (TruthFrames.batch: TrainingFrames.batch + one more kernel, ia_sample_truth) against
TrainingFrames.batch on the same resident frames, the evaluation datum of a large frame, and the constructor's passes (valid rectangle,
downscale).  Device-timed (events), warm-up, medians; everything comes from ONE run; the numbers are reported, nothing is asserted on them.

    python tools/truth_batch_bench.py [--frames 100] [--height 180] [--width 320] [--rays 4096] [--calls 50] [--out profiles/truth_frames.json]
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


def timed(fn, calls, warmup=5):
    """median device time of one call: an event pair around each of `calls` calls after the warm-up"""
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in pairs), out


def synthetic(F, H, W, dev, seed):
    """a moving ellipse per frame (about a fifth of the pixels) and three patterned uint8 images, generated on the device"""
    y, x = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    f = torch.arange(F, device=dev)[:, None, None]
    cx = W * (0.45 + 0.1 * torch.sin(0.3 * f.float()))
    masks = ((((x - cx) / (0.17 * W)) ** 2 + ((y - 0.52 * H) / (0.4 * H)) ** 2) <= 1).float()
    img = lambda s: torch.stack([(x * 3 + y * 5 + f + s) % 256, (x * 7 + y * 2 + 40 * f + s) % 256, (x + y * y + f + s) % 256], -1).to(torch.uint8)      # noqa: E731
    return img(seed), img(seed + 50), img(seed + 100), masks


def frames_for(data, F, H, W, dev, sampler, truth):
    images, albedos, normals, masks = synthetic(F, H, W, dev, 1)
    K = np.array([[1500.0 * W / 1080, 0, W / 2], [0, 1500.0 * W / 1080, H / 2], [0, 0, 1]])
    smpl = dict(betas=np.zeros(10), body_pose=np.zeros((F, 69)), global_orient=np.zeros((F, 3)), transl=np.tile([0.0, 0.2, 2.6], (F, 1)))
    if not truth:
        return data.TrainingFrames(images, masks, K, np.eye(4), smpl, sampler, near=1.0, far=4.0)
    return data.TruthFrames(images, masks, K, np.eye(4), smpl, sampler, near=1.0, far=4.0, albedos=albedos, normals=normals, w2c=np.eye(4),
                            valid_dilate=100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--height", type=int, default=180)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "truth_frames.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times the MI355X: it does not run without one"
    from intrinsicavatar_amd import build, data
    build.build()
    dev = torch.device("cuda:0")
    F, H, W, n = a.frames, a.height, a.width, a.rays
    smp = data.EdgeSampler(n, 0.6, 0.3, 16)                            # configs/sampler/edge.yaml
    plain, truth = frames_for(data, F, H, W, dev, smp, False), frames_for(data, F, H, W, dev, smp, True)
    frame = F // 2
    words = torch.randint(0, 2 ** 63 - 1, (n,), dtype=torch.int64, device=dev)
    plain_ms, p = timed(lambda: plain.batch(frame, words=words), a.calls)
    truth_ms, t = timed(lambda: truth.batch(frame, words=words), a.calls)
    plain_draw_ms, _ = timed(lambda: plain.batch(frame), a.calls)
    truth_draw_ms, _ = timed(lambda: truth.batch(frame), a.calls)
    truth.check(t)
    shared_equal = all(bool(torch.equal(p[k], t[k])) for k in p)
    rect_ms, _ = timed(lambda: data.valid_rect(truth.masks, 100), a.calls)

    big = frames_for(data, 2, 720, 1280, dev, None, True)              # the evaluation datum of a 720 x 1280 frame (H x W)
    full_ms, full = timed(lambda: big.full_frame(1), a.calls)
    plain_big = frames_for(data, 2, 720, 1280, dev, None, False)
    full_plain_ms, _ = timed(lambda: plain_big.full_frame(1), a.calls)
    rect_big_ms, _ = timed(lambda: data.valid_rect(big.masks, 100), a.calls)

    src_u8, _, _, src_f32 = synthetic(8, 720, 1280, dev, 3)
    down = {}
    for s in (2, 4):
        down[f"u8_s{s}_ms"], out_u8 = timed(lambda: data.downscale_center(src_u8, s), a.calls)
        down[f"f32_s{s}_ms"], _ = timed(lambda: data.downscale_center(src_f32, s), a.calls)
        traffic = src_u8.numel() * 4 / (s * s) + out_u8.numel()      # four source bytes per output byte, + the output
        down[f"u8_s{s}_algorithmic_GBps"] = traffic / down[f"u8_s{s}_ms"] / 1e6
    res = {"device": torch.cuda.get_device_name(0), "timing": f"device events around each of {a.calls} calls after 5 warm-up calls, median",
           "batch": {"frames": F, "height": H, "width": W, "rays": n, "sampler": "EdgeSampler(0.6, 0.3, 16)",
                     "training_frames_given_words_ms": plain_ms, "truth_frames_given_words_ms": truth_ms,
                     "extra_given_words_ms": truth_ms - plain_ms,
                     "training_frames_ms": plain_draw_ms, "truth_frames_ms": truth_draw_ms, "extra_ms": truth_draw_ms - plain_draw_ms,
                     "extra_output_bytes": n * (12 + 12 + 1), "shared_keys_equal": shared_equal},
           "full_frame": {"height": 720, "width": 1280, "truth_frames_ms": full_ms, "training_frames_ms": full_plain_ms,
                          "valid_pixels": int(full["valid_mask"].sum())},
           "constructor": {"valid_rect_ms": rect_ms, "valid_rect_frames": F, "valid_rect_720x1280_2_frames_ms": rect_big_ms,
                           "downscale_8_frames_720x1280": down}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
