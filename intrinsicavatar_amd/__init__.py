"""intrinsicavatar_amd -- MI355X (gfx950) implementation of IntrinsicAvatar's volumetric
render_step hot path, exposed through the operator surface the reference imports:

    intrinsicavatar_amd.nerfacc       <- `nerfacc` (traverse_grids, render_weight_from_alpha, ...)
    intrinsicavatar_amd.lib_nerfacc   <- `lib.nerfacc` (ray_resampling*, pack/unpack)
    intrinsicavatar_amd.fast_snarf    <- fast-SNARF JIT modules (fuse_broyden, filter, precompute)
    intrinsicavatar_amd.tinycudann    <- `tinycudann` (Encoding: HashGrid / SphericalHarmonics, incl. double backward)
    intrinsicavatar_amd.pbr           <- `lib.torch_pbr` (emitter / scatterer classes, colour helpers) + the fused estimators and the
                                         kernels behind models/pbr/utils.py sample_volume_interaction
    intrinsicavatar_amd.pytorch3d_ops <- `lib.pytorch3d.ops` (knn_points, knn_gather)
    intrinsicavatar_amd.volrend       <- `models/volrend.py` (rendering, rendering_with_normals_sdf, rendering_with_normals_mats_sdf)
    intrinsicavatar_amd.data          <- `datasets/peoplesnapshot.py` + `utils/sampler.py` (make_rays, EdgeSampler / UniformSampler, the
                                         training datum from frames resident on the device)

All compute runs in hand-written HIP kernels behind the C ABI of include/ia_amd.h
(libia_amd.so); PyTorch is used for device memory, streams and torch.distributed only.
"""
__version__ = "0.1.0"

import os as _os

# Host tuning (opt-in): HIP_FORCE_DEV_KERNARG=1 keeps kernel arguments in device memory (a shorter launch path of the HIP runtime; read
# when the runtime initialises, i.e. at the process's first device call).  The path issues hundreds of launches per step: the reference's
# 4096-ray training step 21.4 -> 20.8 ms, the headline step 309.5 -> 307.5 ms (same box, alternating, profiles/r05_dev_kernarg.txt).
# It is a process-wide setting that child processes inherit, so importing the package does NOT write it: the entry points (bench.py,
# __graft_entry__.py, tools/) set it themselves before HIP initialises, a host application exports it, and
# IA_HOST_TUNING=1 makes this import do it.
if _os.environ.get("IA_HOST_TUNING") == "1":
    _os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")


def install_aliases() -> None:
    """make the reference's own import statements resolve to this package:
    `import nerfacc`, `from nerfacc.volrend import ...`, `from lib.nerfacc import ...`, `import tinycudann as tcnn`,
    `from lib.pytorch3d import ops`.
    Call it before the reference's modules are imported (top of launch.py / sitecustomize.py)."""
    import sys
    import types
    from . import lib_nerfacc, nerfacc, pbr, pytorch3d_ops, tinycudann
    sys.modules["nerfacc"] = nerfacc
    sys.modules["nerfacc.volrend"] = nerfacc
    lib = sys.modules.get("lib") or types.ModuleType("lib")
    lib.nerfacc = lib_nerfacc
    sys.modules["lib"] = lib
    sys.modules["lib.nerfacc"] = lib_nerfacc
    lib.torch_pbr = pbr                     # the eleven classes of models/__init__.py:39-51 + rgb_to_srgb, luminance, luma, max_value
    sys.modules["lib.torch_pbr"] = pbr
    sys.modules["tinycudann"] = tinycudann
    p3d = sys.modules.get("lib.pytorch3d") or types.ModuleType("lib.pytorch3d")      # `from lib.pytorch3d import ops` (deformer_torch.py:1)
    p3d.ops = pytorch3d_ops
    lib.pytorch3d = p3d
    sys.modules["lib.pytorch3d"] = p3d
    sys.modules["lib.pytorch3d.ops"] = pytorch3d_ops
