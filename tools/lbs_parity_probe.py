"""Measure the differences the forward-skinning and vertex-normal tests are held to, and write tests/golden/lbs_parity_bars.json.

    python tools/lbs_parity_probe.py [--out tests/golden/lbs_parity_bars.json]      (on the MI355X: host replay + GPU)
    python tools/lbs_parity_probe.py --host-only                                    (no GPU: refreshes "host_replay", keeps the GPU part)

host_replay   tests/lbs_harness.c (gcc, csrc/lbs_math.h) against tests/golden/golden_lbs*.npz (w, xd, R: the reference's own
              query_weights closure + skinning_mask on the CPU) and against the fp64 numpy normals of the fixture mesh
gpu_observed  ia_forward_skinning / mesh.vertex_normals / mesh.pose on the device against the same references; normal_permuted = the
              normals of the fixture mesh with its face array permuted; pose_identity_xd / _normal = the fixture mesh (scaled into the
              grid's box) posed with identity transforms against the canonical vertices / the fp64 normals of the posed vertices;
              pose_rigid_xd / pose_rigid_normal = one rigid transform on all 24 bones against the transformed vertices / rotated normals
gpu           3 x gpu_observed: what tests/test_gpu_lbs.py asserts, under the hard ceilings of tests/test_lbs_cpu.py's docstring
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import test_lbs_cpu as H      # noqa: E402

COMMENT = ("max abs differences; written by tools/lbs_parity_probe.py. host_replay: tests/lbs_harness.c against tests/golden/golden_lbs*.npz "
           "(w, xd, R) and against fp64 numpy (normal). gpu_observed: the MI355X against the same references (pose_*: mesh.pose of the fixture "
           "mesh against the transformed canonical mesh). gpu = 3 x gpu_observed, asserted by tests/test_gpu_lbs.py under the hard ceilings "
           "stated in tests/test_lbs_cpu.py.")


def fixture_deformer(g, dev):
    """a SNARFDeformer on the fixture's grid"""
    import torch
    from intrinsicavatar_amd.deformer import SNARFDeformer
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    return SNARFDeformer(T(g["grid"]), T(g["offset_kernel"]), T(g["scale_kernel"]), T(g["bbox"]))


def measure_gpu(g, dev="cuda:0"):
    import torch
    from intrinsicavatar_amd import mesh
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    d = fixture_deformer(g, dev)
    d.tfs = T(g["tfs"])[None]
    xd, R, w = d.forward_skinning(T(g["xc"]), want_weights=True)
    m = {"w": float(np.abs(w.cpu().numpy().astype(np.float64) - g["w"]).max()),
         "xd": float(np.abs(xd.cpu().numpy().astype(np.float64) - g["xd"]).max()),
         "R": float(np.abs(R.cpu().numpy().astype(np.float64) - g["R"]).max())}
    nrm = mesh.vertex_normals(T(g["mesh_v"]), T(g["mesh_f"])).cpu().numpy()
    m["normal"] = float(np.abs(nrm.astype(np.float64) - H.normals_fp64(g["mesh_v"], g["mesh_f"])).max())
    fp = H.permuted_faces(g["mesh_f"])
    nrm = mesh.vertex_normals(T(g["mesh_v"]), T(fp)).cpu().numpy()
    m["normal_permuted"] = float(np.abs(nrm.astype(np.float64) - H.normals_fp64(g["mesh_v"], g["mesh_f"])).max())
    v, f = H.mesh_in_box(g)
    cano = {"v_pos": T(v), "t_pos_idx": T(f)}
    d.tfs = torch.eye(4, device=dev).expand(1, 24, 4, 4).contiguous()
    posed = mesh.pose(cano, d)
    m["pose_identity_xd"] = float(np.abs(posed["v_pos"].cpu().numpy().astype(np.float64) - v).max())
    m["pose_identity_normal"] = float(np.abs(posed["v_nrm"].cpu().numpy().astype(np.float64)
                                             - H.normals_fp64(posed["v_pos"].cpu().numpy(), f)).max())
    A = H.rigid_transform().astype(np.float64)
    d.tfs = T(A.astype(np.float32))[None, None].expand(1, 24, 4, 4).contiguous()
    posed = mesh.pose(cano, d)
    want_v = v.astype(np.float64) @ A[:3, :3].T + A[:3, 3]
    want_n = H.normals_fp64(v, f) @ A[:3, :3].T
    m["pose_rigid_xd"] = float(np.abs(posed["v_pos"].cpu().numpy().astype(np.float64) - want_v).max())
    m["pose_rigid_normal"] = float(np.abs(posed["v_nrm"].cpu().numpy().astype(np.float64) - want_n).max())
    return m


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lbs_parity_bars.json"))
    ap.add_argument("--host-only", action="store_true", help="no GPU here: refresh host_replay, keep the GPU part of --out as it is")
    a = ap.parse_args(argv)
    g = H.load_golden()
    h = H.build_harness(tempfile.mkdtemp(prefix="lbs_probe_"))
    out = {"_comment": COMMENT, "host_replay": H.measure_host(h, g)}
    if a.host_only:
        old = json.load(open(a.out)) if os.path.exists(a.out) else {}
        out.update({k: old[k] for k in ("gpu_observed", "gpu") if k in old})
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("no GPU: the GPU part of the bars is measured on the MI355X (or pass --host-only)")
        obs = measure_gpu(g)
        out["gpu_observed"] = obs
        out["gpu"] = {k: 3 * v for k, v in obs.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=2)
        fh.write("\n")
    print(json.dumps(out, indent=2))
    return 0


if __name__ == "__main__":
    sys.exit(main())
