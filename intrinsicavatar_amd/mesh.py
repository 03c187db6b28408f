"""Canonical mesh export: the isosurface of the SDF by marching cubes on the GPU (models/rf/geometry.py:14-104,
models/intrinsic_avatar.py:277-279 and 1685-1701, systems/intrinsic_avatar.py:923-930).

    marching_cubes(level, threshold, vmin, vmax)   MarchingCubeHelper.forward (+ isosurface_'s vertex scaling) on a device grid
    isosurface(geometry, resolution, chunk, threshold)
                                                   BaseImplicitGeometry.isosurface: coarse pass over the geometry's bbox, fine pass
                                                   over the coarse mesh's extent grown by 10 % (clamped to the bbox)
    export(geometry, export_config)                IntrinsicAvatar.export: the mesh alone (the reference attaches no vertex colour)
    vertex_normals(v_pos, t_pos_idx)               area-weighted vertex normals [V,3], bit-reproducible (csrc/mesh_attr.hip)
    skinning_weights(mesh, deformer)               [V,24] skinning weights of the vertices (the deformer's grid, csrc/lbs_fwd.hip)
    pose(mesh, deformer)                           the mesh skinned with the deformer's prepared pose + its normals there

The grid points, the SDF (VolumeSDF.sdf_only, chunk by chunk) and the extraction (csrc/mcubes.hip) stay on the device; a marching-cubes
call reads back its two output sizes once, isosurface() additionally the coarse mesh's extent (6 floats).  Conventions of the
extraction: csrc/mc_math.h and DESIGN.md "Mesh export".

    python -m intrinsicavatar_amd.mesh --state-dict CKPT --bbox x0 y0 z0 x1 y1 z1 [--resolution 512] [--global-step 25000] --out mesh.obj
    python -m intrinsicavatar_amd.mesh --state-dict CKPT --smpl-npz BODY.npz [--cano-pose A_pose] ... --out mesh.obj
    ... --normals                                  `vn` lines in the .obj
    ... --smpl-npz BODY.npz --pose-npz POSES.npz --frame K [--skinned-npz OUT.npz]
                                                   the mesh posed for frame K of POSES.npz (body_pose [F,69], global_orient [F,3], transl [F,3])
"""
import argparse
import ctypes as C
import sys
from typing import Dict, Optional, Sequence

import torch

from . import _lib as L

# configs/geometry/progressive_hash_grid.yaml:6-10
ISOSURFACE = dict(method="mc", resolution=512, chunk=2097152, threshold=0.0)


def _box(vmin, vmax):
    lo = [0.0, 0.0, 0.0] if vmin is None else [float(v) for v in vmin]
    hi = [1.0, 1.0, 1.0] if vmax is None else [float(v) for v in vmax]
    return (C.c_float * 6)(*lo, *hi)


@torch.no_grad()
def marching_cubes(level: torch.Tensor, threshold: float = 0.0, vmin: Optional[Sequence[float]] = None,
                   vmax: Optional[Sequence[float]] = None) -> Dict[str, torch.Tensor]:
    """level [nx,ny,nz] fp32 on the GPU -> {"v_pos": [V,3] fp32, "t_pos_idx": [T,3] int64} on the same device.
    mcubes.marching_cubes(-level, threshold): a grid point is inside iff -level > threshold; vertices are index coordinates / (n - 1),
    then scale_anything((0,1) -> (vmin, vmax)) per axis when a box is given (float32 values)."""
    if level.dim() != 3 or min(level.shape) < 2:
        raise ValueError(f"marching_cubes needs a [nx, ny, nz] grid with every side >= 2, got {tuple(level.shape)}")
    if level.dtype != torch.float32:
        raise TypeError("marching_cubes needs a float32 level grid")
    level = level.contiguous()
    nx, ny, nz = (int(s) for s in level.shape)
    dev = level.device
    scratch = L.work_area(L.lib().ia_mc_scratch_bytes(nx, ny, nz), dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    thr = float(threshold)
    L.lib().ia_mc_count(nx, ny, nz, level, thr, scratch, totals)
    n_v, n_t = (int(v) for v in totals.tolist())             # the one read-back: sizes of the outputs
    if n_v >= 2 ** 31:
        raise ValueError(f"marching_cubes: {n_v} vertices do not fit the int32 vertex-id table")
    v_pos = torch.empty((n_v, 3), dtype=torch.float32, device=dev)
    t_pos_idx = torch.empty((n_t, 3), dtype=torch.int64, device=dev)
    if n_v > 0:
        first_vid = torch.empty(nx * ny * nz, dtype=torch.int32, device=dev)
        L.lib().ia_mc_emit(nx, ny, nz, level, thr, _box(vmin, vmax), scratch, first_vid, v_pos, t_pos_idx)
    return {"v_pos": v_pos, "t_pos_idx": t_pos_idx}


def grid_axes(resolution: int, vmin: torch.Tensor, vmax: torch.Tensor) -> torch.Tensor:
    """[3, R] float32 (host): isosurface_'s scale_anything(linspace(0, 1, R), (0, 1), (vmin[a], vmax[a])) per axis -- the coordinates
    the reference's meshgrid combines, element for element."""
    lin = torch.linspace(0, 1, resolution)
    return torch.stack([((lin - 0) / (1 - 0)) * (vmax[a] - vmin[a]) + vmin[a] for a in range(3)])


def fine_bbox(vmin: torch.Tensor, vmax: torch.Tensor, bbox: torch.Tensor):
    """BaseImplicitGeometry.isosurface: the coarse mesh's extent grown by 10 % of itself, clamped to the bbox (float32, host)."""
    vmin_ = (vmin - (vmax - vmin) * 0.1).clamp(bbox[0], bbox[1])
    vmax_ = (vmax + (vmax - vmin) * 0.1).clamp(bbox[0], bbox[1])
    return vmin_, vmax_


@torch.no_grad()
def level_grid(geometry, resolution: int, vmin: torch.Tensor, vmax: torch.Tensor, chunk: int = ISOSURFACE["chunk"]) -> torch.Tensor:
    """SDF of the R^3 grid over [vmin, vmax] ([R,R,R] fp32 on the geometry's device): grid points straight into the hash grid's
    normalized coordinates (ia_mc_grid_points), then VolumeSDF.sdf_only chunk by chunk (values do not depend on the chunk)."""
    R = int(resolution)
    dev = geometry.center.device
    axes = grid_axes(R, vmin, vmax).reshape(-1).to(dev)
    n = R ** 3
    level = torch.empty(n, dtype=torch.float32, device=dev)
    chunk = max(1, min(int(chunk), n))
    xp = torch.empty((chunk, 3), dtype=torch.float32, device=dev)
    center, scale = geometry.center.contiguous().float(), geometry.scale.contiguous().float()
    for start in range(0, n, chunk):
        m = min(chunk, n - start)
        L.lib().ia_mc_grid_points(m, start, R, R, R, axes, center, scale, xp)
        level[start:start + m] = geometry.sdf_only(xp[:m], normalized=True)
    return level.view(R, R, R)


@torch.no_grad()
def isosurface_(geometry, vmin: torch.Tensor, vmax: torch.Tensor, resolution: int = ISOSURFACE["resolution"],
                chunk: int = ISOSURFACE["chunk"], threshold: float = ISOSURFACE["threshold"]) -> Dict[str, torch.Tensor]:
    """one pass of BaseImplicitGeometry.isosurface_ over the box [vmin, vmax] (float32 [3] host tensors)."""
    level = level_grid(geometry, resolution, vmin, vmax, chunk)
    return marching_cubes(level, threshold, vmin.tolist(), vmax.tolist())


@torch.no_grad()
def isosurface(geometry, resolution: int = ISOSURFACE["resolution"], chunk: int = ISOSURFACE["chunk"],
               threshold: float = ISOSURFACE["threshold"]) -> Dict[str, torch.Tensor]:
    """BaseImplicitGeometry.isosurface: the fine-pass mesh {"v_pos", "t_pos_idx"} on the geometry's device.  geometry.bbox is the
    deformer's canonical bbox (prepare_bbox).  Raises ValueError when the coarse pass finds no surface."""
    bbox = geometry.bbox.detach().float().cpu()
    coarse = isosurface_(geometry, bbox[0], bbox[1], resolution, chunk, threshold)
    if coarse["v_pos"].shape[0] == 0:
        raise ValueError("isosurface: the coarse pass found no surface inside the bbox")
    ext = torch.stack([coarse["v_pos"].amin(dim=0), coarse["v_pos"].amax(dim=0)]).cpu()     # 6 floats, reduced on the device
    del coarse
    vmin_, vmax_ = fine_bbox(ext[0], ext[1], bbox)
    return isosurface_(geometry, vmin_, vmax_, resolution, chunk, threshold)


@torch.no_grad()
def export(geometry, export_config=None) -> Dict[str, torch.Tensor]:
    """IntrinsicAvatar.export: geometry.isosurface().  export_config (`export_vertex_color`, `chunk_size`) is accepted and changes nothing:
    the reference computes vertex features for export_vertex_color, then attaches no colour (its v_rgb lines are commented out), so the
    mesh is v_pos + t_pos_idx either way."""
    return geometry.isosurface()


def vertex_faces(n_vertices: int, t_pos_idx: torch.Tensor):
    """the vertex -> incident-faces lists of a triangle mesh as CSR: (offsets int32 [V+1], lists int32 [3T]); lists[offsets[v] ..
    offsets[v+1]) holds the faces at vertex v in no particular order (vertex_normals sorts them).  Integer atomics + the library's
    exclusive scan; a face with an index outside [0, V) is in no list."""
    if not t_pos_idx.is_cuda:
        raise L.IaError("mesh.vertex_faces needs GPU tensors (no CPU fallback)")
    faces = t_pos_idx.reshape(-1, 3).contiguous().to(torch.int64)
    V, T = int(n_vertices), int(faces.shape[0])
    dev = faces.device
    offsets = torch.empty(V + 1, dtype=torch.int32, device=dev)
    L.lib().ia_mesh_vertex_faces_count(T, V, faces, offsets)
    L.lib().ia_exclusive_scan_i32(offsets, offsets, None, V + 1, L.scan_tmp(V + 1, dev))
    cursor = torch.empty(max(V, 1), dtype=torch.int32, device=dev)
    lists = torch.empty(max(3 * T, 1), dtype=torch.int32, device=dev)
    L.lib().ia_mesh_vertex_faces_fill(T, V, faces, offsets, cursor, lists)
    return offsets, lists[:3 * T]


@torch.no_grad()
def vertex_normals(v_pos: torch.Tensor, t_pos_idx: torch.Tensor, return_lists: bool = False):
    """area-weighted vertex normals [V,3] fp32 of the mesh v_pos [V,3], t_pos_idx [T,3]: the sum of the un-normalised
    (v1 - v0) x (v2 - v0) over the faces at the vertex, in ascending face index, then n / max(|n|, 1e-12).  No float atomics: two runs,
    and runs on differently scheduled devices, give the same bits (csrc/mesh_attr.hip, csrc/lbs_math.h).  A vertex of no face gets 0.
    return_lists: (v_nrm, offsets int32 [V+1], lists int32 [3T]) with every vertex's list sorted."""
    if not v_pos.is_cuda:
        raise L.IaError("mesh.vertex_normals needs GPU tensors (no CPU fallback)")
    if v_pos.dim() != 2 or v_pos.shape[1] != 3 or t_pos_idx.dim() != 2 or t_pos_idx.shape[1] != 3:
        raise ValueError(f"vertex_normals needs v_pos [V,3] and t_pos_idx [T,3], got {tuple(v_pos.shape)} and {tuple(t_pos_idx.shape)}")
    v = v_pos.detach().contiguous().float()
    faces = t_pos_idx.contiguous().to(torch.int64)
    V, T = int(v.shape[0]), int(faces.shape[0])
    offsets, lists = vertex_faces(V, faces)
    v_nrm = torch.empty((V, 3), dtype=torch.float32, device=v.device)
    L.lib().ia_mesh_vertex_normals(V, T, v, faces, offsets, lists, v_nrm)
    return (v_nrm, offsets, lists) if return_lists else v_nrm


@torch.no_grad()
def skinning_weights(mesh: Dict[str, torch.Tensor], deformer) -> torch.Tensor:
    """[V,24] skinning weights of the mesh's vertices: the deformer's weight grid at v_pos (SNARFDeformer.query_weights)."""
    return deformer.query_weights(mesh["v_pos"])


@torch.no_grad()
def pose(mesh: Dict[str, torch.Tensor], deformer) -> Dict[str, torch.Tensor]:
    """the canonical mesh in the deformer's prepared pose (deformer.prepare(tfs, w2s)): v_pos skinned forward with deformer.tfs
    (SNARFDeformer.forward_skinning; SMPL-root frame, as tfs is), the faces shared with `mesh` (not copied), and v_nrm = the vertex
    normals of the posed surface (vertex_normals of the posed vertices)."""
    xd, _ = deformer.forward_skinning(mesh["v_pos"], want_rot=False)
    return {"v_pos": xd, "t_pos_idx": mesh["t_pos_idx"], "v_nrm": vertex_normals(xd, mesh["t_pos_idx"])}


def _smpl_npz_body(path: str, device="cpu", dtype=torch.float64):
    """(smpl.SMPLKinematics, betas [1,NB]) of the body stored in an .npz (the arrays SMPLKinematics takes, plus betas)."""
    import numpy as np
    from . import smpl
    z = np.load(path)
    missing = [k for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "parents", "lbs_weights", "betas") if k not in z.files]
    if missing:
        raise SystemExit(f"{path}: missing arrays {missing}")
    t = lambda k: torch.from_numpy(np.asarray(z[k], dtype=np.float64)).to(device=device, dtype=dtype)      # noqa: E731
    body = smpl.SMPLKinematics(t("v_template"), t("shapedirs"), t("posedirs"), t("J_regressor"), z["parents"].tolist(), t("lbs_weights"))
    return body, t("betas").reshape(-1, body.shapedirs.shape[-1])[:1]


def _cano_pose_arg(cano_pose):
    if isinstance(cano_pose, str) and "," in cano_pose:
        return [float(v) for v in cano_pose.split(",")]
    return cano_pose


def smpl_npz_deformer(smpl_npz: str, pose_npz: str, frame: int, cano_pose="A_pose", device="cuda:0", resolution: int = 128):
    """the deformer of the body in `smpl_npz`, prepared for frame `frame` of `pose_npz` (body_pose [F,69], global_orient [F,3],
    transl [F,3]): deformer.initialize, then smpl.SMPLKinematics.forward + smpl.deformer_transforms + deformer.prepare
    (SNARFDeformer.initialize / prepare_deformer, snarf_deformer.py:46-126).  -> (deformer, tfs [1,24,4,4])"""
    import numpy as np
    from . import deformer as D, smpl
    body, betas = _smpl_npz_body(smpl_npz, device=device, dtype=torch.float32)
    z = np.load(pose_npz)
    missing = [k for k in ("body_pose", "global_orient", "transl") if k not in z.files]
    if missing:
        raise SystemExit(f"{pose_npz}: missing arrays {missing}")
    F = z["body_pose"].shape[0]
    if not 0 <= frame < F:
        raise SystemExit(f"{pose_npz}: --frame {frame} outside 0 .. {F - 1}")
    t = lambda k: torch.from_numpy(np.asarray(z[k][frame:frame + 1], dtype=np.float32)).reshape(1, -1).to(device)      # noqa: E731
    dfm, A_rest_inv, _, _ = D.initialize(body, betas, _cano_pose_arg(cano_pose), resolution=resolution)
    out = body.forward(betas, t("body_pose"), t("global_orient"), t("transl"))
    tfs, w2s = smpl.deformer_transforms(out["A"], A_rest_inv)
    dfm.prepare(tfs, w2s[0])
    return dfm, tfs


def smpl_npz_bbox(path: str, cano_pose="A_pose") -> torch.Tensor:
    """[2,3] float32 canonical bbox of the body stored in an .npz (the arrays smpl.SMPLKinematics takes, plus betas): the body in its
    canonical pose, then smpl.bbox_from_vertices (SNARFDeformer.initialize, snarf_deformer.py:46-71).  24 joints on the host."""
    from . import smpl
    body, betas = _smpl_npz_body(path)
    cano_pose = _cano_pose_arg(cano_pose)
    out = body.forward(betas, smpl.rest_pose(cano_pose).double(), torch.zeros((1, 3), dtype=torch.float64))
    return smpl.bbox_from_vertices(out["vertices"].float())


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m intrinsicavatar_amd.mesh",
                                 description="canonical-space mesh (.obj) of the SDF of a reference-layout checkpoint")
    ap.add_argument("--state-dict", required=True, help="Lightning checkpoint ({'state_dict': ...}) or a plain state dict")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--bbox", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                     help="canonical bbox of the deformer (not part of the state dict)")
    src.add_argument("--smpl-npz", metavar="FILE", help="body model arrays (v_template, shapedirs, posedirs, J_regressor, parents, "
                     "lbs_weights) plus betas: the bbox is that of the body in its canonical pose (smpl.bbox_from_vertices)")
    ap.add_argument("--cano-pose", default="A_pose", help="canonical pose of --smpl-npz: a predefined name or four comma-separated numbers")
    ap.add_argument("--resolution", type=int, default=ISOSURFACE["resolution"])
    ap.add_argument("--chunk", type=int, default=ISOSURFACE["chunk"])
    ap.add_argument("--threshold", type=float, default=ISOSURFACE["threshold"])
    ap.add_argument("--global-step", type=int, default=25000, help="step of the progressive hash-level mask")
    ap.add_argument("--prefix", default="model.")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", required=True)
    ap.add_argument("--normals", action="store_true", help="write area-weighted vertex normals (`vn` lines, `f a//a b//b c//c`)")
    ap.add_argument("--pose-npz", metavar="FILE", help="pose the mesh: body_pose [F,69], global_orient [F,3], transl [F,3]; the body "
                    "comes from --smpl-npz, its bone transforms through smpl.SMPLKinematics + smpl.deformer_transforms")
    ap.add_argument("--frame", type=int, default=0, help="frame of --pose-npz")
    ap.add_argument("--skinned-npz", metavar="FILE", help="also write the animatable form (vertices, faces, normals, [V,24] skinning "
                    "weights, the frame's bone transforms): needs --pose-npz")
    a = ap.parse_args(argv)
    if a.pose_npz is not None and a.smpl_npz is None:
        ap.error("--pose-npz needs the body of --smpl-npz")
    if a.skinned_npz is not None and a.pose_npz is None:
        ap.error("--skinned-npz needs --pose-npz")
    from . import checkpoint, fields, io_formats
    ck = torch.load(a.state_dict, map_location="cpu", weights_only=False)       # a Lightning file also pickles its hyper-parameters
    sd = ck.get("state_dict", ck)
    parts = checkpoint.split_reference_state_dict(sd, a.prefix)
    if "geometry" not in parts:
        raise SystemExit(f"{a.state_dict}: no '{a.prefix}geometry.*' entries")
    geo = fields.VolumeSDF(seed=None)
    geo.load_state_dict(parts["geometry"], strict=True)
    geo = geo.to(a.device)
    bbox = torch.tensor(a.bbox, dtype=torch.float32).view(2, 3) if a.bbox is not None else smpl_npz_bbox(a.smpl_npz, a.cano_pose)
    geo.prepare_bbox(bbox.to(a.device))
    geo.update_step(0, a.global_step)
    mesh = isosurface(geo, a.resolution, a.chunk, a.threshold)
    if a.pose_npz is not None:
        dfm, tfs = smpl_npz_deformer(a.smpl_npz, a.pose_npz, a.frame, a.cano_pose, a.device)
        if a.skinned_npz is not None:
            cano = dict(mesh, v_nrm=vertex_normals(mesh["v_pos"], mesh["t_pos_idx"]))
            io_formats.save_skinned_npz(a.skinned_npz, cano, skinning_weights(mesh, dfm), tfs[0])
        mesh = pose(mesh, dfm)
    elif a.normals:
        mesh["v_nrm"] = vertex_normals(mesh["v_pos"], mesh["t_pos_idx"])
    io_formats.save_obj(a.out, mesh["v_pos"], mesh["t_pos_idx"], mesh["v_nrm"] if a.normals else None)
    print(f"{a.out}: {mesh['v_pos'].shape[0]} vertices, {mesh['t_pos_idx'].shape[0]} faces")
    return 0


if __name__ == "__main__":
    sys.exit(main())
