#!/usr/bin/env python3
"""Same-box A/B of two builds of libia_amd.so on the level-major hash gather: parent against candidate, alternating, every
measurement a fresh child process that loads its library through IA_AMD_LIB.

  probe : tools/sdf_head_probe.py on IA_N sorted points (one SDF-only query = 12 gather launches), --reps alternations
  pmc   : `rocprofv3 --pmc` passes of that probe, counters alone (no tracing alongside), one pass per counter group and build
  bench : `bench.py --gpus 1 --steps S --warmup W` (headline step), --reps alternations, parent and candidate only
--also adds builds of variants to the probe and pmc stages.

Each stage merges its section into --out (JSON), so the stages may run in separate invocations.  A child that ends with a
signal or a time limit ends the run: nothing more is started on the device.

  python tools/hash_gather_ab.py --parent _ab/libia_amd_parent.so --cand intrinsicavatar_amd/libia_amd.so \
      --stages probe pmc bench --out profiles/hash_gather_pair_loads.json
"""
import argparse
import collections
import csv
import glob
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATHER = "hash_fwd_xcd_kernel<false>"
PMC_GROUPS = (["TCP_TOTAL_CACHE_ACCESSES_sum", "TCP_TCC_READ_REQ_sum", "GRBM_GUI_ACTIVE"], ["TCC_HIT_sum", "TCC_MISS_sum"])


def sha16(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


def child(cmd, lib, limit, log, extra_env=None):
    env = dict(os.environ, IA_AMD_LIB=os.path.abspath(lib), **(extra_env or {}))
    try:
        p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"{' '.join(cmd)}: no end after {limit} s -- stopping")
    text = p.stdout.decode(errors="replace")
    if log:
        with open(log, "w") as fh:
            fh.write(text)
    if p.returncode != 0 or "illegal memory access" in text or "Memory access fault" in text:
        sys.exit(f"{' '.join(cmd)}: exit status {p.returncode} -- stopping\n{text[-2000:]}")
    return text


def last_json(text):
    for line in reversed(text.splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise RuntimeError("no JSON line:\n" + text[-2000:])


def stage_probe(a, libs, logs):
    rows = []
    for rep in range(a.reps):
        for name, lib in libs.items():
            r = last_json(child([sys.executable, "tools/sdf_head_probe.py"], lib, 300, f"{logs}/probe_{name}_{rep}.log", {"IA_N": str(a.points)}))
            rows.append(dict(build=name, rep=rep, ms_per_query=r))
            print(name, rep, r["ia_hashgrid_fwd_xcd"], flush=True)
    series = {n: [r["ms_per_query"]["ia_hashgrid_fwd_xcd"] for r in rows if r["build"] == n] for n in libs}
    return dict(points=a.points, gather_launches_per_query=12, note="ms per SDF-only query and entry point, mean of 3 queries after 2 warm-up "
                "queries in each process (device events); rows in run order", rows=rows, gather_ms=series,
                every_candidate_run_beats_every_parent_run=max(series["candidate"]) < min(series["parent"]),
                parent_spread_percent=round(100 * (max(series["parent"]) - min(series["parent"])) / min(series["parent"]), 2))


def stage_pmc(a, libs, logs):
    out = {}
    for name, lib in libs.items():
        per, launches = collections.defaultdict(float), 0
        for gi, group in enumerate(PMC_GROUPS):
            d = f"{logs}/pmc_{name}_{gi}"
            child(["rocprofv3", "--pmc", *group, "--output-format", "csv", "-d", d, "--", sys.executable, "tools/sdf_head_probe.py"], lib, 600,
                  f"{logs}/pmc_{name}_{gi}.log", {"IA_N": str(a.points)})
            f = glob.glob(d + "/**/*counter_collection.csv", recursive=True)
            seen = set()
            for r in csv.DictReader(open(f[0])):
                if GATHER not in r["Kernel_Name"].replace("(anonymous namespace)::", ""):
                    continue
                per[r["Counter_Name"]] += float(r["Counter_Value"])
                seen.add(r.get("Dispatch_Id"))
            launches = len(seen)
        row = {k: v / launches for k, v in per.items()}
        row["launches"] = launches
        row["l2_hit_rate"] = row["TCC_HIT_sum"] / (row["TCC_HIT_sum"] + row["TCC_MISS_sum"])
        row["l1_hit_rate"] = 1.0 - row["TCP_TCC_READ_REQ_sum"] / row["TCP_TOTAL_CACHE_ACCESSES_sum"]
        out[name] = row
        print(name, row, flush=True)
    out["note"] = (f"counters per launch of {GATHER} (mean over the launches of 5 queries of {a.points} points: dense set + 11 hashed levels), "
                   "one rocprofv3 --pmc pass per counter group, nothing traced alongside")
    out["accesses_candidate_over_parent"] = out["candidate"]["TCP_TOTAL_CACHE_ACCESSES_sum"] / out["parent"]["TCP_TOTAL_CACHE_ACCESSES_sum"]
    return out


def stage_bench(a, libs, logs):
    libs = {n: libs[n] for n in ("parent", "candidate")}
    rows = []
    for rep in range(a.reps):
        for name, lib in libs.items():
            r = last_json(child([sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup)], lib, 900,
                                f"{logs}/bench_{name}_{rep}.log"))
            rows.append(dict(build=name, rep=rep, ms_per_step=r["ms_per_step"], value=r["value"], unit=r["unit"]))
            print(name, rep, r["ms_per_step"], flush=True)
    series = {n: [r["ms_per_step"] for r in rows if r["build"] == n] for n in libs}
    mean = {n: sum(v) / len(v) for n, v in series.items()}
    return dict(command=f"bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup}", rows=rows, ms_per_step=series, mean_ms_per_step=mean,
                gain_ms=mean["parent"] - mean["candidate"], parent_spread_ms=max(series["parent"]) - min(series["parent"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--cand", required=True)
    ap.add_argument("--stages", nargs="+", choices=["probe", "pmc", "bench"], default=["probe", "pmc", "bench"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hash_gather_pair_loads.json"))
    ap.add_argument("--logs", default=os.path.join(ROOT, "_ab", "hash_gather_ab_logs"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resources", default=None, help="JSON file with the code-object notes of the gather kernel (vgpr_count, scratch, LDS) per build")
    ap.add_argument("--also", nargs="*", default=[], metavar="NAME=LIB", help="further builds for the probe and pmc stages (variants measured and not kept)")
    a = ap.parse_args()
    libs = dict(parent=a.parent, candidate=a.cand, **dict(v.split("=", 1) for v in a.also))
    a.logs = os.path.abspath(a.logs)
    os.makedirs(a.logs, exist_ok=True)
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out["libraries_sha256_16"] = {n: sha16(p) for n, p in libs.items()}
    sys.path.insert(0, ROOT)
    from intrinsicavatar_amd import build
    out["tree_library_sources_sha256_16"] = build.source_fingerprint()
    if a.resources:
        out["code_object_notes"] = json.load(open(a.resources))
    for s in a.stages:
        out[s] = dict(probe=stage_probe, pmc=stage_pmc, bench=stage_bench)[s](a, libs, a.logs)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
