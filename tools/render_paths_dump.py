"""A/B of the host code that strings the render kernels together: dump what every render path returns, compare two commits.

  python tools/render_paths_dump.py dump OUT_DIR
      runs every scenario below on the 40 x 40 synthetic frame of tests/test_gpu_headline_call.py and writes, per scenario,
      OUT_DIR/<scenario>.npz (every tensor of the returned dict, nested dicts included, and every parameter's .grad) and
      OUT_DIR/calls.json (the C-ABI entry points called, with their call counts and units; and, from a second run of the scenario
      under torch.profiler, the names of ALL device kernels and copies in launch order, ATen's included).  Uses only entry points that are
      old, so the same file runs in a checkout of an earlier commit (it imports the package of the checkout it lies in).
  python tools/render_paths_dump.py compare --parent P1 P2 P3 P4 --child C [C2 ...] [--bench FILE] --out profiles/render_paths_ab.json
      an array the parent runs reproduce bit for bit must be bit-identical in the child; any other one (atomics in the backward
      kernels) may differ from a parent run -- the NEAREST one: min over the parent runs of the largest absolute difference -- by at
      most twice the largest pairwise difference among the parent runs; the entry-point names, counts and units must be equal, and
      so must the device kernels launched, as a multiset; whether their ORDER is the parent's too is reported per scenario.  Exit status 1 if anything is outside.  Further child runs and the
      parent runs judged against each other are reported as evidence of how often the bound is missed by chance.

All random inputs come from ONE seeded generator, scenario by scenario in a fixed order."""
import argparse
import itertools
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"


def flatten(o, prefix=""):
    import torch
    out = {}
    for k, v in o.items():
        if isinstance(v, dict):
            out.update(flatten(v, f"{prefix}{k}/"))
        elif isinstance(v, torch.Tensor):
            out[prefix + k] = v.detach().cpu().numpy()
        elif isinstance(v, (int, float)) and not isinstance(v, bool):
            out[prefix + k] = np.asarray(v)
    return out


def dump(out_dir):
    import torch
    from torch.profiler import profile, ProfilerActivity
    from intrinsicavatar_amd import _lib as L, build, fields, pbr, synthetic as S
    build.build()
    os.makedirs(out_dir, exist_ok=True)
    rs, rays, _ = S.build_frame(DEV, 40, 40, pose_seed=0, beta=0.05, num_samples_per_ray=64, grid_D=16, grid_H=64, grid_W=64,
                                smooth_iters=5, hash_amp=1e-2)
    mat = fields.VolumeMaterial(seed=2).to(DEV)
    sg = pbr.EnvironmentLightSG(num_SGs=12, base_res=16, seed=4).to(DEV)
    env = pbr.EnvironmentLightTensor(sg.generate_image().detach())
    env.update_pdf()
    n = rays.shape[0]
    g = torch.Generator().manual_seed(20)
    U = lambda *shape: torch.rand(shape, generator=g).to(DEV)      # noqa: E731
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    named = [(f"rs{i}", p) for i, p in enumerate(rs.parameters())] + [(f"mat{i}", p) for i, p in enumerate(mat.parameters()) if p.requires_grad]
    calls, kernels = {}, {}

    def run(name, fn, extra_grads=()):
        for _, p in named:
            p.grad = None
        L.lib().start()
        o = fn()
        rep = L.lib().report(detail=True)
        arrays = flatten(o)
        for k, p in list(named) + list(extra_grads):
            if p.grad is not None:
                arrays["grad/" + k] = p.grad.detach().cpu().numpy()
        np.savez(os.path.join(out_dir, name + ".npz"), **arrays)
        calls[name] = {k: [len(v), [u for _, u, _ in v]] for k, v in sorted(rep.items())}
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev_evs = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        kernels[name] = [e.name[:90] for e in sorted(dev_evs, key=lambda e: e.time_range.start)]
        print(f"{name}: {len(arrays)} arrays, {sum(c[0] for c in calls[name].values())} entry-point calls, {len(kernels[name])} device launches", flush=True)

    def eval_scenarios(tag):
        jit = U(n)
        run("forward" + tag, lambda: rs.forward(rays, jit))
        lu, su = U(512, 3), U(n, 512)
        run("relight_light" + tag, lambda: rs.relight(rays, mat, env, 64, lu[:64].contiguous(), su[:, :64].contiguous(), background_color=bg,
                                                     global_illumination=True, jitter=jit, add_emitter=True))
        run("relight_uniform_light" + tag, lambda: rs.relight(rays, mat, env, 512, lu, su, background_color=bg, global_illumination=True,
                                                             render_mode="uniform_light", return_index_lists=True))
        sc, ratio = U(n * 64, 6), torch.tensor([0.9, 1.1, 1.05], device=DEV)
        run("relight_mats" + tag, lambda: rs.relight(rays, mat, env, 64, lu[:64].contiguous(), su[:, :64].contiguous(), global_illumination=True,
                                                    render_mode="mats", scatter_u=sc, albedo_align_ratio=ratio))
        run("relight_mis" + tag, lambda: rs.relight(rays, mat, env, 64, lu[:64].contiguous(), su[:, :64].contiguous(), background_color=bg,
                                                   global_illumination=True, render_mode="mis", scatter_u=sc))
        run("forward_" + tag, lambda: rs.forward_(rays, mat, env, 512, lu, su, background_color=bg, global_illumination=True,
                                                  render_mode="uniform_light", jitter=jit))

    eval_scenarios("")
    jit, curv, mj = U(n), U(n * 128, 3), torch.randn((n * 128, 3), generator=g).to(DEV)
    run("forward_train_rf_", lambda: rs.forward_train_rf_(rays, jit, curv, bg))
    lu_pp, lu, su = U(n * 64, 3), U(512, 3), U(n, 512)
    run("forward_train_light", lambda: rs.forward_train_(rays, mat, env, 64, lu_pp, jitter=jit, background_color=bg, global_illumination=True,
                                                         render_mode="light"))
    leaf = sg.generate_image().detach().requires_grad_(True)
    run("forward_train_uniform_light", lambda: rs.forward_train_(
        rays, mat, env, 512, lu, jitter=jit, material_jitter=mj, background_color=bg, global_illumination=True, render_mode="uniform_light",
        shuffle_u=su, env_base=leaf, add_emitter=True, curv_u=curv))
    target, tmask = U(n, 3), (U(n) > 0.5).float()
    run("forward_backward", lambda: rs.forward_backward(rays, target, tmask, jitter=jit, curv_u=curv, lambda_curv=0.05))
    tfs = rs.deformer.tfs
    tfs.requires_grad_(True)
    tfs.grad = None
    run("forward_backward_pose", lambda: rs.forward_backward(rays, target, tmask, jitter=jit, curv_u=curv, lambda_curv=0.05), [("tfs", tfs)])
    tfs.requires_grad_(False)
    run("forward_backward_phys", lambda: rs.forward_backward_phys(rays, target, mat, env, 512, lu, su, target_mask=tmask, jitter=jit,
                                                                 background_color=bg, global_illumination=True))
    lam = dict(lambda_rgb_l1=1.0, lambda_rgb_phys_l1=1.0, lambda_rgb_demodulated=0.1, lambda_eikonal=0.1, lambda_mask_bce=0.1,
               lambda_sparsity=0.01, sparsity_scale=1.0, lambda_albedo_smoothness=0.01, lambda_normal_orientation=0.01)
    leaf.grad = None
    run("forward_backward_phys_loss_config", lambda: rs.forward_backward_phys(
        rays, target, mat, env, 64, lu_pp, None, target_mask=tmask, jitter=jit, render_mode="light", env_base=leaf, background_color=bg,
        global_illumination=True, light_sampling="per_point", material_jitter=mj, loss_config=lam), [("env_base", leaf)])
    rs.SORT_MIN_POINTS = 1          # the sorted branches of _sdf_at and _secondary_chunks at this size
    eval_scenarios("_sorted")
    with open(os.path.join(out_dir, "calls.json"), "w") as f:
        json.dump(calls, f, default=str)
    with open(os.path.join(out_dir, "kernels.json"), "w") as f:
        json.dump(kernels, f)


def maxdiff(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return float("inf")
    if a.tobytes() == b.tobytes():
        return 0.0
    a, b = a.astype(np.float64), b.astype(np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    d = np.abs(np.where(both_nan, 0.0, a) - np.where(both_nan, 0.0, b))
    return float("inf") if np.isnan(d).any() else float(d.max())


def compare(parents, children, bench, out):
    """the rule is applied to the FIRST child run; further child runs are evidence: their own outside arrays, and per scenario the largest
    ratio of a child-to-child and of a child-to-parent difference to the parent spread (same code = same distribution = ratios alike)."""
    calls = [json.load(open(os.path.join(d, "calls.json"))) for d in parents + children]
    kern = [json.load(open(os.path.join(d, "kernels.json"))) for d in parents + children]
    summary, ok = {}, True
    for name in calls[0]:
        P = [np.load(os.path.join(d, name + ".npz")) for d in parents]
        Cs = [np.load(os.path.join(d, name + ".npz")) for d in children]
        s = dict(arrays=0, bit_identical=0, within_parent_spread=0, outside=[], outside_in_further_child_runs=[],
                 parent_runs_over_twice_the_spread_of_the_other_parent_runs=0, largest_child_to_child_over_parent_spread=0.0,
                 largest_child_to_parent_over_parent_spread=0.0,
                 entry_points_equal=all(c.get(name) == calls[0][name] for c in calls[1:]),
                 device_launches=len(kern[0][name]), parent_kernel_sequences_agree=all(k[name] == kern[0][name] for k in kern[1:len(parents)]),
                 keys_equal=all(list(p.files) == list(C.files) for p in P for C in Cs))      # same keys in the same ORDER
        for k in P[0].files:
            s["arrays"] += 1
            pair = {(i, j): maxdiff(P[i][k], P[j][k]) for i, j in itertools.combinations(range(len(P)), 2)}
            spread = max(pair.values(), default=0.0)
            diffs = [[maxdiff(C[k], p[k]) for p in P] if k in C.files else [float("inf")] for C in Cs]
            if spread == 0.0 and max(diffs[0]) == 0.0:
                s["bit_identical"] += 1
            elif spread > 0.0 and min(diffs[0]) <= 2.0 * spread:       # "differs from a parent run by at most twice the largest pairwise difference"
                s["within_parent_spread"] += 1
            else:
                s["outside"].append(dict(array=k, parent_spread=spread, child_diffs=diffs[0]))
            for n, d in enumerate(diffs[1:], 2):
                if not (max(d) == 0.0 if spread == 0.0 else min(d) <= 2.0 * spread):
                    s["outside_in_further_child_runs"].append(dict(child_run=n, array=k, parent_spread=spread, child_diffs=d))
            if spread > 0.0:
                cc = max([maxdiff(a[k], b[k]) for a, b in itertools.combinations(Cs, 2)], default=0.0)
                s["largest_child_to_child_over_parent_spread"] = max(s["largest_child_to_child_over_parent_spread"], round(cc / spread, 3))
                s["largest_child_to_parent_over_parent_spread"] = max(s["largest_child_to_parent_over_parent_spread"],
                                                                      round(max(max(d) for d in diffs) / spread, 3))
            # how often a PARENT run lies farther than the bound from every other parent run, judged by the spread of the runs without it
            for i in range(len(P)) if len(P) > 2 else ():
                rest = max(v for ij, v in pair.items() if i not in ij)
                s["parent_runs_over_twice_the_spread_of_the_other_parent_runs"] += int(min(v for ij, v in pair.items() if i in ij) > 2.0 * rest > 0.0)
        s["kernel_sequence_equal"] = all(k[name] == kern[0][name] for k in kern[len(parents):])
        s["kernels_launched_equal"] = all(sorted(k[name]) == sorted(kern[0][name]) for k in kern[1:])
        ok = ok and not s["outside"] and s["entry_points_equal"] and s["keys_equal"] and s["kernels_launched_equal"]
        summary[name] = s
    res = dict(parent_runs=len(parents), child_runs=len(children), scenarios=summary, all_pass=ok)
    if bench:
        res["bench"] = json.load(open(bench))
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for k, v in summary.items():
        print(k, v["arrays"], v["bit_identical"], v["within_parent_spread"], "outside:", [(o["array"], o["parent_spread"], o["child_diffs"]) for o in v["outside"]],
              "further:", [(o["child_run"], o["array"]) for o in v["outside_in_further_child_runs"]],
              v["parent_runs_over_twice_the_spread_of_the_other_parent_runs"], v["largest_child_to_child_over_parent_spread"],
              v["largest_child_to_parent_over_parent_spread"], v["entry_points_equal"], v["keys_equal"], v["device_launches"],
              v["parent_kernel_sequences_agree"], v["kernel_sequence_equal"], v["kernels_launched_equal"])
    print("all pass" if ok else "OUTSIDE THE BOUND")
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("dump").add_argument("out_dir")
    c = sub.add_parser("compare")
    c.add_argument("--parent", nargs="+", required=True)
    c.add_argument("--child", nargs="+", required=True)
    c.add_argument("--bench")
    c.add_argument("--out", required=True)
    a = ap.parse_args()
    sys.exit(dump(a.out_dir) or 0 if a.cmd == "dump" else compare(a.parent, a.child, a.bench, a.out))
