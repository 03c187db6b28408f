"""Build libia_amd.so (all gfx950 kernels + the C ABI of include/ia_amd.h) with hipcc.

hipcc cross-compiles for gfx950 without a GPU.  The library is written IN-TREE
(intrinsicavatar_amd/libia_amd.so) so that it travels to the GPU box with the repo.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "_obj")
SO = os.path.join(HERE, "libia_amd.so")

COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-fno-fast-math"]
# Translation units whose float comparisons decide integer outputs are built WITHOUT
# fma contraction so they reproduce the oracle bit-for-bit; the field kernels
# (hash grid / MLP, tolerance-checked) use fma.
SOURCES = {
    "core.hip": [],
    "traverse.hip": ["-ffp-contract=off"],
    "composite.hip": ["-ffp-contract=off"],
    "resample.hip": ["-ffp-contract=off"],
    "snarf.hip": ["-ffp-contract=off"],
    "hashgrid.hip": ["-munsafe-fp-atomics"],
    "mlp.hip": [],
    "mlp_bwd.hip": ["-munsafe-fp-atomics"],
    "mlp_train.hip": ["-munsafe-fp-atomics"],
    "deform.hip": ["-ffp-contract=off"],
    "pbr.hip": ["-munsafe-fp-atomics"],
    "volint.hip": ["-ffp-contract=off"],
    "sort.hip": ["-ffp-contract=off"],
    "occgrid.hip": [],
    "optim.hip": ["-ffp-contract=off"],
    "stepops.hip": ["-ffp-contract=off"],
    "mcubes.hip": ["-ffp-contract=off"],
    "metrics.hip": ["-ffp-contract=off"],
    "skinning.hip": ["-ffp-contract=off"],
    "data.hip": ["-ffp-contract=off"],
    "lbs_fwd.hip": ["-ffp-contract=off"],
    "mesh_attr.hip": ["-ffp-contract=off"],
    "train_loss.hip": ["-ffp-contract=off"],
    "lpips.hip": ["-ffp-contract=off"],
    "pose_terms.hip": ["-ffp-contract=off"],
}


def source_fingerprint() -> str:
    """sha256 (first 16 hex digits) over every kernel source, header and compiler flag that goes into libia_amd.so: the library is
    rebuilt whenever this differs from the fingerprint recorded next to it (mtimes do not survive a copy of the tree), and
    bench.py reports it so that a measured library can be tied to the sources that are tracked."""
    import hashlib
    h = hashlib.sha256()
    h.update(repr(COMMON).encode())
    files = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))]
    files.append(os.path.join(os.path.dirname(HERE), "include", "ia_amd.h"))
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(repr(SOURCES.get(os.path.basename(f), "")).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


FINGERPRINT = SO + ".src"        # sidecar of the built library (git-ignored like the library, travels with it)


def built_fingerprint():
    try:
        return open(FINGERPRINT).read().strip()
    except OSError:
        return None


def _stale(dst, srcs):
    if not os.path.exists(dst):
        return True
    t = os.path.getmtime(dst)
    return any(os.path.getmtime(s) > t for s in srcs if os.path.exists(s))


def build(force: bool = False, verbose: bool = False) -> str:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OBJ, exist_ok=True)
    fp = source_fingerprint()
    if os.path.exists(SO) and built_fingerprint() != fp:
        force = True                     # the library next to these sources was built from other sources (or nobody knows from which)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(os.path.dirname(HERE), "include", "ia_amd.h"))
    objs, procs = [], []
    for src, extra in SOURCES.items():
        s = os.path.join(CSRC, src)
        if not os.path.exists(s):
            continue
        o = os.path.join(OBJ, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + headers):
            cmd = [hipcc] + COMMON + extra + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd))
            procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    failed = False
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            failed = True
            sys.stderr.write(f"--- hipcc failed on {src}\n{out.decode(errors='replace')}\n")
        elif verbose and out:
            print(out.decode(errors="replace"))
    if failed:
        raise RuntimeError("hipcc failed")
    if force or procs or _stale(SO, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO] + objs
        subprocess.check_call(cmd)
    if built_fingerprint() != fp:
        with open(FINGERPRINT, "w") as fh:
            fh.write(fp + "\n")
    return SO


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
