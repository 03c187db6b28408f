"""Time the construction of the deformer from a body surface (SNARFDeformer.from_smpl) per stage at resolution 128 and 256, next to the
same construction written with torch operators on the device (chunked pairwise distances + topk, gather + sum, the slice expression
of the sweeps) -- what a user of the package had before.  Device-timed (events), warm-up, medians over repeats.

    python tools/deformer_init_bench.py [--repeats 5] [--out profiles/deformer_init.json]
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

K = 30


def timed(fn, repeats, warmup=1):
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


def torch_knn(x, verts, chunk=32768):
    d2s, idxs = [], []
    for s in range(0, x.shape[0], chunk):
        d = x[s:s + chunk, None, :] - verts[None]
        d2 = (d * d).sum(-1)
        v, i = torch.topk(d2, K, dim=1, largest=False, sorted=True)
        d2s.append(v)
        idxs.append(i)
    return torch.cat(d2s), torch.cat(idxs)


def torch_blend(d2, idx, W, chunk=65536):
    out = []
    for s in range(0, d2.shape[0], chunk):
        dist = d2[s:s + chunk].sqrt().clamp_(0.0001, 1.)
        ws = 1. / dist
        ws = ws / ws.sum(-1, keepdim=True)
        out.append((ws[..., None] * W[idx[s:s + chunk]]).sum(-2))
    return torch.cat(out).T.contiguous()


def torch_smooth(weights, sweeps=30):
    weights = weights[None].clone()
    for _ in range(sweeps):
        mean = (weights[:, :, 2:, 1:-1, 1:-1] + weights[:, :, :-2, 1:-1, 1:-1] + weights[:, :, 1:-1, 2:, 1:-1]
                + weights[:, :, 1:-1, :-2, 1:-1] + weights[:, :, 1:-1, 1:-1, 2:] + weights[:, :, 1:-1, 1:-1, :-2]) / 6.0
        weights[:, :, 1:-1, 1:-1, 1:-1] = (weights[:, :, 1:-1, 1:-1, 1:-1] - mean) * 0.7 + mean
        weights = weights / weights.sum(1, keepdim=True)
    return weights[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deformer_init.json"))
    a = ap.parse_args()
    from intrinsicavatar_amd import fast_snarf, pytorch3d_ops
    from intrinsicavatar_amd.deformer import SNARFDeformer
    dev = "cuda:0"
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden_skinning.npz"))
    verts = torch.from_numpy(z["verts"]).to(dev)
    Wn = np.zeros((verts.shape[0], 24), np.float32)
    for c in range(4):
        np.add.at(Wn, (np.arange(Wn.shape[0]), z["w_idx"][:, c].astype(np.int64)), z["w_val"][:, c])
    W = torch.from_numpy(Wn).to(dev)
    scale, offset = float(z["scale"]), z["offset"].tolist()
    res = {"device": torch.cuda.get_device_name(0), "V": int(verts.shape[0]), "K": K, "repeats": a.repeats, "timing": "device events, median",
           "resolutions": {}}
    for R in a.resolutions:
        D = R // 4
        P = D * R * R
        r = {"queries": P, "pairs": P * int(verts.shape[0])}
        hip, tor = {}, {}
        hip["grid_points_ms"], x = timed(lambda: fast_snarf.skin_grid_points(D, R, R, 4.0, scale, offset, dev), a.repeats)
        hip["knn_ms"], (d2, idx) = timed(lambda: pytorch3d_ops.knn_points_flat(x, verts, K), a.repeats)
        hip["blend_ms"], blend = timed(lambda: fast_snarf.skin_blend(d2, idx, W), a.repeats)
        hip["smooth_30_ms"], grid = timed(lambda: fast_snarf.skin_smooth(blend.view(24, D, R, R), 30), a.repeats)
        hip["from_smpl_ms"], _ = timed(lambda: SNARFDeformer.from_smpl(verts[None], W[None], resolution=R), a.repeats)
        hip["knn_pairs_per_s"] = r["pairs"] / (hip["knn_ms"] * 1e-3)
        tor["knn_ms"], (td2, tidx) = timed(lambda: torch_knn(x, verts), a.repeats)
        tor["blend_ms"], tblend = timed(lambda: torch_blend(td2, tidx, W), a.repeats)
        tor["smooth_30_ms"], tgrid = timed(lambda: torch_smooth(tblend.view(24, D, R, R)), a.repeats)
        tor["total_ms"] = tor["knn_ms"] + tor["blend_ms"] + tor["smooth_30_ms"]
        hip["stages_total_ms"] = hip["grid_points_ms"] + hip["knn_ms"] + hip["blend_ms"] + hip["smooth_30_ms"]
        r["agreement"] = {"idx_rows_equal_to_torch_topk": float((tidx.int() == idx).all(1).float().mean()),
                          "grid_max_abs_diff_to_torch": float((tgrid - grid).abs().max())}
        # what bounds the k-NN: 8 float32 operations per pair (3 sub, 3 mul, 2 add) + the compare, no memory traffic to speak of
        r["knn_flops_per_s"] = 8 * hip["knn_pairs_per_s"]
        r["hip"], r["torch"] = hip, tor
        r["speedup_total"] = tor["total_ms"] / hip["stages_total_ms"]
        res["resolutions"][str(R)] = r
        del x, d2, idx, blend, grid, td2, tidx, tblend, tgrid
        torch.cuda.empty_cache()
    print(json.dumps(res))
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
