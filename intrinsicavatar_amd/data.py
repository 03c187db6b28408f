"""Training batches on the device: camera rays, the pixel samplers and the dataset datum (datasets/peoplesnapshot.py:19-33 and
:49-175, utils/sampler.py:9-67) on frames that stay resident in HBM.

    make_rays(K, c2w, H, W, device)          make_rays: (rays_o [H,W,3], rays_d [H,W,3]) float32, fp64 arithmetic
    EdgeSampler / UniformSampler             the reference's constructor arguments, asserts and int() splits; EdgeSampler.edge_band
    TrainingFrames(images, masks, K, c2w, smpl_params, sampler, near, far)
        .batch(idx, generator, words)        PeopleSnapshotDataset.__getitem__ (train) as the DataLoader collates it at batch_size 1
        .full_frame(idx)                     the evaluation form: every pixel in order
        .check(batch)                        one read-back of the status word -> the reference's ValueError
    TrainingFrames.from_peoplesnapshot(root, split, start, end, skip, ...)
    AnimationFrames.from_dir(root, betas, start, end, skip, downscale, hdri_filepath, near, far)
        .frame(idx)                          AnimationDataset.__getitem__ (test split, datasets/animation.py:50-206) collated at batch size 1
    animation_host(root, betas, start, end, ...)   its host-only part: files, K, translation, near / far (no GPU)
    TruthFrames(TrainingFrames arguments, albedos=, normals=, w2c=, valid_dilate=, hdri_files=, near_far=)
        .batch / .full_frame                 the datum of datasets/rana.py / synthetichuman.py: + albedo, normal, valid_mask, w2c (+ hdri)
    TruthFrames.from_rana / .from_synthetichuman(data_root, subject, split, start, end, skip, ..., downscale)
    truth_host(kind, data_root, subject, split, start, end, ...)   their host-only part (no GPU)
    valid_rect(masks, k), downscale_center(x, s)   the constructor's passes on the device (DESIGN.md "Ground-truth frames")

A step costs torch.randint plus one kernel (csrc/data.hip: ia_sample_batch) and no host synchronisation; the samplers' index lists
(np.where(mask), np.where(mask_o - mask_i)) are built once per dataset in the constructor, whose one read-back sizes them.

The edge band follows the reference AS WRITTEN: EdgeSampler.sample flattens the mask before cv2.erode / cv2.dilate (utils/sampler.py:27-31),
so the morphology runs over an N x 1 image -- one 1-D window of kernel_size taps over the flat row-major pixel index, which wraps
across image rows.  That is the default.  EdgeSampler(..., two_dimensional=True) runs the window over rows, then columns of [H, W]
instead, which is what the constructor's square kernel suggests.  Conventions and what is unverified: DESIGN.md "Training batches".

The draws are np.random.randint(0, n) replayed as word % n over non-negative int64 words (torch.randint(0, 2**63 - 1) on the device, or
recorded words).  BalancedSampler and PatchSampler draw with np.random.choice(replace=False), a permutation that cannot be replayed
from recorded words without restating numpy's generator: their names raise NotImplementedError.
"""
import ctypes as C
import glob
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib as L

MAX_KERNEL_SIZE = 64      # csrc/data_math.h: IA_WINDOW_MAX_K


def _need_gpu(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise L.IaError("intrinsicavatar_amd operators need GPU tensors (no CPU fallback)")
    return device


def camera_words(K, c2w):
    """the 21 doubles the kernels take (HOST): inv(K) [9], c2w[:3,:3] [9], c2w[:3,3] [3]; the cameras are taken as float64."""
    K, c2w = np.asarray(K, np.float64), np.asarray(c2w, np.float64)
    if K.shape != (3, 3) or c2w.shape[-1] != 4 or c2w.shape[0] < 3:
        raise ValueError(f"need K [3,3] and c2w [4,4] (or [3,4]), got {K.shape} and {c2w.shape}")
    vals = np.concatenate([np.linalg.inv(K).reshape(-1), c2w[:3, :3].reshape(-1), c2w[:3, 3].reshape(-1)])
    return (C.c_double * 21)(*[float(v) for v in vals])


def make_rays(K, c2w, H: int, W: int, device) -> Tuple[Tensor, Tensor]:
    """make_rays (datasets/peoplesnapshot.py:25-33) on the device: (rays_o, rays_d), both [H,W,3] float32."""
    device = _need_gpu(device)
    H, W = int(H), int(W)
    rays_o = torch.empty((H, W, 3), dtype=torch.float32, device=device)
    rays_d = torch.empty((H, W, 3), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        L.lib().ia_make_rays(H * W, None, H, W, camera_words(K, c2w), rays_o, rays_d)
    return rays_o, rays_d


def window_minmax(x: Tensor, k: int, dim: int = -1) -> Tuple[Tensor, Tensor]:
    """minimum and maximum of float32 `x` over the k taps at offsets -(k/2) ... k - 1 - k/2 along `dim`, taps outside ignored: the
    rectangular cv2.erode / cv2.dilate along one axis.  -> (min, max), shaped like x."""
    if not x.is_cuda:
        raise L.IaError("intrinsicavatar_amd operators need GPU tensors (no CPU fallback)")
    if x.dtype != torch.float32:
        raise TypeError("window_minmax needs float32")
    x = x.contiguous()
    dim = dim % x.dim()
    outer = int(np.prod(x.shape[:dim], dtype=np.int64))
    inner = int(np.prod(x.shape[dim + 1:], dtype=np.int64))
    lo, hi = torch.empty_like(x), torch.empty_like(x)
    with torch.cuda.device(x.device):
        L.lib().ia_window_minmax(outer, x.shape[dim], inner, int(k), x, lo, hi)
    return lo, hi


class UniformSampler:
    """utils/sampler.py:52-67: num_sample pixels drawn uniformly over the frame."""

    def __init__(self, num_sample):
        self.num_sample = num_sample
        self.num_mask = 0
        self.num_edge = 0
        self.num_rand = num_sample


class EdgeSampler:
    """utils/sampler.py:9-49: int(num_sample * ratio_mask) pixels from the mask, int(num_sample * ratio_edge) from the edge band
    dilate(mask) - erode(mask), the rest uniform over the frame.

    The edge band follows the reference as written: `sample` flattens the mask before the morphology, so the kernel_size window runs
    over the FLAT row-major pixel index (an N x 1 image) and wraps across image rows.  two_dimensional=True runs it over the rows, then
    the columns of [H, W] instead -- the square kernel the constructor builds."""

    def __init__(self, num_sample, ratio_mask=0.6, ratio_edge=0.3, kernel_size=32, two_dimensional=False):
        assert ratio_mask >= 0.0
        assert ratio_edge >= 0.0
        assert ratio_edge + ratio_mask <= 1.0
        if not 1 <= int(kernel_size) <= MAX_KERNEL_SIZE:
            raise ValueError(f"kernel_size must be in [1, {MAX_KERNEL_SIZE}], got {kernel_size}")
        self.kernel_size = int(kernel_size)
        self.two_dimensional = bool(two_dimensional)
        self.num_sample = num_sample
        self.num_mask = int(num_sample * ratio_mask)
        self.num_edge = int(num_sample * ratio_edge)
        self.num_rand = num_sample - self.num_mask - self.num_edge

    def edge_band(self, mask: Tensor) -> Tuple[Tensor, Tensor]:
        """mask [H,W] or [F,H,W] float32 on the GPU -> (mask_i, mask_o) = (erode, dilate) of every frame, shaped like mask."""
        if mask.dim() not in (2, 3):
            raise ValueError(f"edge_band needs [H,W] or [F,H,W], got {tuple(mask.shape)}")
        if not self.two_dimensional:
            flat = mask.reshape(-1, mask.shape[-2] * mask.shape[-1]) if mask.dim() == 3 else mask.reshape(-1)
            lo, hi = window_minmax(flat, self.kernel_size, -1)
            return lo.view(mask.shape), hi.view(mask.shape)
        row_lo, row_hi = window_minmax(mask, self.kernel_size, -1)
        return window_minmax(row_lo, self.kernel_size, -2)[0], window_minmax(row_hi, self.kernel_size, -2)[1]


def _unreplayable(name):
    class _Sampler:
        def __init__(self, *a, **kw):
            raise NotImplementedError(f"{name} draws with np.random.choice(replace=False): a permutation that cannot be replayed from "
                                      "recorded words without restating numpy's generator")
    _Sampler.__name__ = _Sampler.__qualname__ = name
    return _Sampler


BalancedSampler = _unreplayable("BalancedSampler")
PatchSampler = _unreplayable("PatchSampler")

# the `_target_` names of configs/sampler/*.yaml
SAMPLERS = {"utils.sampler.EdgeSampler": EdgeSampler, "utils.sampler.UniformSampler": UniformSampler,
            "utils.sampler.BalancedSampler": BalancedSampler, "utils.sampler.PatchSampler": PatchSampler}


def sampler_from_config(config: dict):
    """hydra.utils.instantiate for a configs/sampler/*.yaml mapping: {"_target_": "utils.sampler.EdgeSampler", "num_sample": 4096, ...}."""
    kw = dict(config)
    return SAMPLERS[kw.pop("_target_")](**kw)


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, Tensor) else np.asarray(a)


class TrainingFrames:
    """A subject's frames on the device.  images uint8 [F,H,W,3] and masks [F,H,W] are GPU tensors; K [3,3], c2w [4,4] and smpl_params
    (betas [10] or [1,10], body_pose [F,69], global_orient [F,3], transl [F,3]) are host arrays or tensors.  near / far: the config's
    values, or (both None) |transl[idx]| -+ 1 as the reference forms them."""

    def __init__(self, images: Tensor, masks: Tensor, K, c2w, smpl_params: Dict, sampler=None, near=None, far=None):
        if not (images.is_cuda and masks.is_cuda):
            raise L.IaError("intrinsicavatar_amd operators need GPU tensors (no CPU fallback)")
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
            raise TypeError(f"images must be uint8 [F,H,W,3], got {images.dtype} {tuple(images.shape)}")
        if masks.shape != images.shape[:3]:
            raise ValueError(f"masks {tuple(masks.shape)} do not match images {tuple(images.shape)}")
        self.device = images.device
        self.F, self.H, self.W = (int(s) for s in images.shape[:3])
        self.images = images.contiguous()
        self.masks = masks.to(torch.float32).contiguous()                    # msk.astype(np.float32)
        self.sampler = sampler
        self.cam = camera_words(K, c2w)
        p = {k: _host(smpl_params[k]).astype(np.float32) for k in ("betas", "body_pose", "global_orient", "transl")}
        for k in ("body_pose", "global_orient", "transl"):
            if p[k].shape[0] != self.F:
                raise ValueError(f"smpl_params[{k!r}] has {p[k].shape[0]} rows for {self.F} frames")
        self.betas = torch.from_numpy(p["betas"].reshape(1, 10)).to(self.device)
        self.body_pose, self.global_orient, self.transl = (torch.from_numpy(np.ascontiguousarray(p[k])).to(self.device)
                                                           for k in ("body_pose", "global_orient", "transl"))
        if near is not None and far is not None:
            near_tab = np.ones(self.F, np.float32) * near                   # np.ones_like(rays_d[..., 0]) * self.near
            far_tab = np.ones(self.F, np.float32) * far
        else:
            dist = np.array([np.sqrt(np.square(p["transl"][i]).sum(-1)) for i in range(self.F)], np.float32)
            near_tab, far_tab = dist - 1, dist + 1
        self.near = torch.from_numpy(near_tab.astype(np.float32)).to(self.device)
        self.far = torch.from_numpy(far_tab.astype(np.float32)).to(self.device)
        self.index = torch.arange(self.F, dtype=torch.int64, device=self.device)
        self.t_idx = torch.tensor([i / self.F for i in range(self.F)], dtype=torch.float64).to(self.device)
        self.mask_start = self.edge_start = self.mask_loc = self.edge_loc = self.counts = None
        if sampler is not None and sampler.num_mask + sampler.num_edge > 0:
            self._build_lists()

    def _build_lists(self):
        F, N = self.F, self.H * self.W
        mask_i, mask_o = self.sampler.edge_band(self.masks)
        dev = self.device
        with torch.cuda.device(dev):
            scratch = L.work_area(L.lib().ia_flag_lists_scratch_bytes(F, N), dev)
            totals = torch.empty(2, dtype=torch.int32, device=dev)
            args = (F, N, self.masks, mask_i, mask_o, scratch)
            L.lib().ia_flag_lists_count(*args, totals)
            n_mask, n_edge = (int(v) for v in totals.tolist())              # the one read-back: sizes of the two lists
            self.mask_start = torch.empty(F + 1, dtype=torch.int32, device=dev)
            self.edge_start = torch.empty(F + 1, dtype=torch.int32, device=dev)
            self.counts = torch.empty((F, 2), dtype=torch.int32, device=dev)
            self.mask_loc = torch.empty(max(n_mask, 1), dtype=torch.int32, device=dev)[:n_mask]
            self.edge_loc = torch.empty(max(n_edge, 1), dtype=torch.int32, device=dev)[:n_edge]
            L.lib().ia_flag_lists_fill(*args, totals, self.mask_start, self.edge_start, self.counts, self.mask_loc, self.edge_loc)

    def __len__(self):
        return self.F

    def _rows(self, idx: int, n: int, num_mask: int, num_edge: int, words: Optional[Tensor]) -> Dict[str, Tensor]:
        idx = int(idx)
        if not 0 <= idx < self.F:
            raise IndexError(f"frame {idx} outside [0, {self.F})")
        dev = self.device
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
        out = {"rgb": f32(1, n, 3), "rays_o": f32(1, n, 3), "rays_d": f32(1, n, 3), "alpha": f32(1, n), "near": f32(1, n), "far": f32(1, n),
               "pixel_indices": torch.empty((1, n), dtype=torch.int64, device=dev), "status": torch.empty(1, dtype=torch.int32, device=dev)}
        with torch.cuda.device(dev):
            L.lib().ia_sample_batch(n, num_mask, num_edge, idx, self.F, self.H, self.W, words, self.masks, self.images, self.mask_start,
                                    self.edge_start, self.mask_loc, self.edge_loc, self.cam, self.near, self.far, out["pixel_indices"], out["alpha"],
                                    out["rgb"], out["rays_o"], out["rays_d"], out["near"], out["far"], out["status"])
        s = slice(idx, idx + 1)
        out.update(betas=self.betas, global_orient=self.global_orient[s], body_pose=self.body_pose[s], transl=self.transl[s],
                   index=self.index[s], t_idx=self.t_idx[s])
        return out

    def batch(self, idx: int, generator: Optional[torch.Generator] = None, words: Optional[Tensor] = None) -> Dict[str, Tensor]:
        """the training datum of frame idx, every entry with the leading dimension of a batch_size-1 DataLoader: rgb, rays_o, rays_d
        [1,n,3], alpha, near, far [1,n], betas [1,10], global_orient [1,3], body_pose [1,69], transl [1,3], index [1] int64, t_idx [1]
        float64 = idx / F, + pixel_indices [1,n] int64 and status [1] int32 (check()).  words [n] int64 >= 0 on the device replay a
        recorded run; otherwise they are drawn with `generator` (a generator of this device).  No host synchronisation."""
        if self.sampler is None:
            raise ValueError("TrainingFrames was built without a sampler: only full_frame() is available")
        n = int(self.sampler.num_sample)
        if words is None:
            words = torch.randint(0, 2 ** 63 - 1, (n,), dtype=torch.int64, device=self.device, generator=generator)
        elif not words.is_cuda:
            raise L.IaError("intrinsicavatar_amd operators need GPU tensors (no CPU fallback)")
        elif words.dtype != torch.int64 or tuple(words.shape) != (n,):
            raise TypeError(f"words must be int64 [{n}], got {words.dtype} {tuple(words.shape)}")
        return self._rows(idx, n, int(self.sampler.num_mask), int(self.sampler.num_edge), words.contiguous())

    def full_frame(self, idx: int) -> Dict[str, Tensor]:
        """the evaluation datum of frame idx: all H * W pixels in order, no sampler (status is 0)."""
        return self._rows(idx, self.H * self.W, 0, 0, None)

    @staticmethod
    def check(batch: Dict[str, Tensor]) -> None:
        """reads the batch's status word (one copy to the host); the reference's np.random.randint(0, 0) raises ValueError."""
        status = int(batch["status"].item())
        if status:
            which = " and ".join(name for bit, name in ((1, "mask"), (2, "edge band")) if status & bit)
            raise ValueError(f"low >= high: the frame's {which} is empty")

    @classmethod
    def from_peoplesnapshot(cls, root: str, split: str, start: int, end: int, skip: int = 1, sampler=None, near=None, far=None,
                            refine: bool = False, downscale=1, device="cuda") -> "TrainingFrames":
        """PeopleSnapshotDataset.__init__ (datasets/peoplesnapshot.py:50-109): cameras.npz, images/*.png (through PIL), masks/*.npy and
        the pose file the reference picks, read once on the host and moved to `device`."""
        if downscale != 1:
            raise NotImplementedError("downscale != 1: every shipped PeopleSnapshot config uses 1, and cv2.resize is not restated here")
        device = _need_gpu(device)
        from PIL import Image
        camera = np.load(os.path.join(root, "cameras.npz"))
        K = camera["intrinsic"]
        c2w = np.linalg.inv(camera["extrinsic"])
        H, W = int(camera["height"]), int(camera["width"])
        sel = slice(start, end + 1, skip)
        img_lists = sorted(glob.glob(f"{root}/images/*.png"))[sel]
        msk_lists = sorted(glob.glob(f"{root}/masks/*.npy"))[sel]
        if refine:
            cached_path = os.path.join(root, "poses/anim_nerf_test.npz")
        elif os.path.exists(os.path.join(root, f"poses/anim_nerf_{split}.npz")):
            cached_path = os.path.join(root, f"poses/anim_nerf_{split}.npz")
        elif os.path.exists(os.path.join(root, f"poses/{split}.npz")):
            cached_path = os.path.join(root, f"poses/{split}.npz")
        else:
            cached_path = None
        cached = bool(cached_path and os.path.exists(cached_path))
        p = dict(np.load(cached_path if cached else os.path.join(root, "poses.npz")))
        if "thetas" in p:
            p["body_pose"], p["global_orient"] = p["thetas"][..., 3:], p["thetas"][..., :3]
        smpl = {k: p[k] if (cached or k == "betas") else p[k][sel] for k in ("betas", "body_pose", "global_orient", "transl")}
        images = np.stack([np.asarray(Image.open(f).convert("RGB"), np.uint8) for f in img_lists])
        masks = np.stack([np.load(f).astype(np.float32) for f in msk_lists])
        if images.shape[1:3] != (H, W):
            raise ValueError(f"images are {images.shape[1:3]}, cameras.npz says {(H, W)}")
        return cls(torch.from_numpy(images).to(device), torch.from_numpy(masks).to(device), K, c2w, smpl, sampler, near, far)


# ----------------------------------------------------------------------------- datasets/animation.py (test split)
def animation_host(root: str, betas, start: int, end: int, skip: int = 1, downscale=1, near=None, far=None) -> Dict:
    """the host-only part of AnimationDataset.__init__ / __getitem__ (datasets/animation.py:50-206, split 'test'): cameras.npz and
    poses.npz, K = diag(2000, 2000, 1) with the principal point (height // 2, width // 2) -- in that order, as the reference writes it --,
    the downscale, transl = trans - trans[0] + (0, 0.15, 5), the [start:end+1:skip] slice, near / far.  No GPU.
    -> dict(K [3,3] float64, height, width, w2c [F,4,4] float32 (a single [4,4] extrinsic repeated), per_frame_extrinsic, betas [1,10],
    body_pose [F,69], global_orient [F,3], transl [F,3], near [F], far [F] float32)."""
    cameras = dict(np.load(os.path.join(root, "cameras.npz")))
    per_frame = cameras["extrinsic"].ndim == 3
    if per_frame:                                                   # height / width are arrays then: the reference takes element 0
        height, width = cameras["height"][0], cameras["width"][0]
    else:
        height, width = cameras["height"], cameras["width"]
    K = np.eye(3)
    K[0, 0] = K[1, 1] = 2000
    K[0, 2] = height // 2
    K[1, 2] = width // 2
    if downscale > 1:
        height, width = int(height / downscale), int(width / downscale)
        K[:2] /= downscale
    sel = slice(start, end + 1, skip)
    p = dict(np.load(os.path.join(root, "poses.npz")))
    thetas = p["poses"][..., :72]
    transl = p["trans"] - p["trans"][0:1]
    transl += (0, 0.15, 5)
    smpl = dict(body_pose=thetas[..., 3:].astype(np.float32)[sel], global_orient=thetas[..., :3].astype(np.float32)[sel],
                transl=transl.astype(np.float32)[sel])
    F = len(smpl["global_orient"])
    ext = cameras["extrinsic"]
    w2c = ext[sel].astype(np.float32) if per_frame else np.repeat(ext.astype(np.float32)[None], F, 0)
    if per_frame and len(w2c) != F:
        raise ValueError(f"{len(w2c)} extrinsics for {F} poses in [{start}:{end + 1}:{skip}]")
    if near is not None and far is not None:
        near_tab, far_tab = np.ones(F, np.float32) * near, np.ones(F, np.float32) * far
    else:
        dist = np.array([np.sqrt(np.square(smpl["transl"][i]).sum(-1)) for i in range(F)], np.float32)
        near_tab, far_tab = dist - 1, dist + 1
    return dict(K=K, height=int(height), width=int(width), w2c=np.ascontiguousarray(w2c), per_frame_extrinsic=bool(per_frame),
                betas=np.asarray(betas).astype(np.float32).reshape(1, 10), near=near_tab.astype(np.float32), far=far_tab.astype(np.float32),
                **smpl)


class AnimationFrames:
    """AnimationDataset, test split, on the device: a motion (poses.npz) seen by one camera or one camera per frame (cameras.npz), lit by
    one HDRI.  `host`: animation_host(...); hdri: [1024,2048,3] float32 (io_formats.load_hdri_2k) or None."""

    def __init__(self, host: Dict, hdri: Optional[np.ndarray] = None, device="cuda"):
        self.device = _need_gpu(device)
        self.host = host
        self.H, self.W, self.F = host["height"], host["width"], len(host["global_orient"])
        self.img_wh = (self.W, self.H)
        dev = self.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        self.betas, self.body_pose, self.global_orient, self.transl = (up(host[k]) for k in ("betas", "body_pose", "global_orient", "transl"))
        self.w2c, self.near, self.far = up(host["w2c"]), up(host["near"]), up(host["far"])
        self.index = torch.arange(self.F, dtype=torch.int64, device=dev)
        self.hdri = None if hdri is None else up(np.asarray(hdri, np.float32))[None]        # loaded once, shared by the frames
        self._rays = {}

    @classmethod
    def from_dir(cls, root: str, betas, start: int, end: int, skip: int = 1, downscale=1, hdri_filepath: Optional[str] = None, near=None,
                 far=None, device="cuda") -> "AnimationFrames":
        hdri = None
        if hdri_filepath is not None:
            assert os.path.exists(hdri_filepath), "HDRI not found: {}".format(hdri_filepath)
            from . import io_formats
            hdri = io_formats.load_hdri_2k(hdri_filepath)
        return cls(animation_host(root, betas, start, end, skip, downscale, near, far), hdri, device)

    def __len__(self):
        return self.F

    def frame(self, idx: int) -> Dict[str, Tensor]:
        """the datum of frame idx with the leading dimension of a batch_size-1 DataLoader: rays_o, rays_d [1,HW,3], betas [1,10],
        global_orient [1,3], body_pose [1,69], transl [1,3], index [1] int64, w2c [1,4,4], near, far [1,HW], hdri [1,1024,2048,3] when a file
        was given.  Rays: ia_make_rays with the frame's c2w = inv(w2c) (float32, as the reference inverts it); a single extrinsic's rays
        are made once."""
        idx = int(idx)
        if not 0 <= idx < self.F:
            raise IndexError(f"frame {idx} outside [0, {self.F})")
        key = idx if self.host["per_frame_extrinsic"] else 0
        if key not in self._rays:
            if len(self._rays) >= 4:
                self._rays.pop(next(iter(self._rays)))
            c2w = np.linalg.inv(self.host["w2c"][idx])                  # float32
            o, d = make_rays(self.host["K"], c2w, self.H, self.W, self.device)
            self._rays[key] = (o.reshape(1, -1, 3), d.reshape(1, -1, 3))
        rays_o, rays_d = self._rays[key]
        s = slice(idx, idx + 1)
        n = self.H * self.W
        out = dict(rays_o=rays_o, rays_d=rays_d, betas=self.betas, global_orient=self.global_orient[s], body_pose=self.body_pose[s],
                   transl=self.transl[s], index=self.index[s], w2c=self.w2c[s], near=self.near[s, None].expand(1, n),
                   far=self.far[s, None].expand(1, n))
        if self.hdri is not None:
            out["hdri"] = self.hdri
        return out


# ----------------------------------------------------------------------------- datasets/rana.py, datasets/synthetichuman.py
TRUTH_KINDS = {"rana": 100, "synthetichuman": 50}       # the side of the valid mask's dilate kernel (rana.py:167, synthetichuman.py:177)


def _center_factor(downscale, height: int, width: int) -> int:
    """the integer factor of a downscale the centre-2x2 rule serves (1: none), NotImplementedError otherwise"""
    s = int(downscale)
    if s != downscale or s < 1 or (s > 1 and (s % 2 or height % s or width % s)):
        raise NotImplementedError(f"downscale {downscale} of {height} x {width}: cv2.resize is restated for 1 and for even integers that "
                                  "divide both sides (the shipped configs use 4, 2 and 1)")
    return s


def truth_host(kind: str, data_root: str, subject: str, split: str, start: int, end: int, skip: int = 1, downscale=1, near=None, far=None,
               refine: bool = False) -> Dict:
    """the host-only part of RANADataset / SyntheticHumanDataset.__init__ and of the per-frame scalars of __getitem__ (datasets/rana.py:
    61-124 and :208-216, datasets/synthetichuman.py:61-134 and :218-228).  No GPU.
    -> dict(kind, root, K [3,3] float32 (rows 0-1 divided by downscale), w2c = RT [4,4] float32, c2w = inv(RT) float32, height, width
    (downscaled), full_height, full_width, img_wh, downscale (int), img_lists, albedo_lists, normal_lists, msk_lists, hdri_files (test
    split, else None), betas [1,10], body_pose [*,69], global_orient [*,3], transl [*,3] float32, near, far [F] float32, dilate_k)."""
    if kind not in TRUTH_KINDS:
        raise ValueError(f"kind must be one of {sorted(TRUTH_KINDS)}, got {kind!r}")
    import json
    rana = kind == "rana"
    root = os.path.join(data_root, split, subject) if rana else os.path.join(data_root, subject)
    with open(os.path.join(root, "cameras.json"), "r") as f:
        camera = json.load(f)
    cam_name = "00"
    if not rana:
        camera = camera[cam_name]
    K = np.array(camera["intrinsic"], dtype=np.float32)
    RT = np.array(camera["extrinsic"], dtype=np.float32)
    c2w = np.linalg.inv(RT)
    full_height, full_width = int(camera["height"]), int(camera["width"])
    s = _center_factor(downscale, full_height, full_width)
    height, width = full_height, full_width
    if s > 1:
        height, width = int(height / s), int(width / s)
        K[:2] /= s
    hdri_files = None
    if split == "test":
        with open(os.path.join(root, "hdri_files.json"), "r") as f:
            hdri_files = [os.path.join(data_root, "hdri", name) for name in json.load(f)]
    sel = slice(start, end + 1, skip)
    sub = "" if rana else f"/{cam_name}"
    img_dir = "images" if rana or split != "test" else "images_relit"
    albedo_dir, normal_dir = ("albedos", "normals") if rana else ("albedos_png", "normals_png")
    lists = {name: sorted(glob.glob(f"{root}/{d}{sub}/*.{ext}"))[sel]
             for name, d, ext in (("img_lists", img_dir, "png"), ("albedo_lists", albedo_dir, "png"), ("normal_lists", normal_dir, "png"),
                                  ("msk_lists", "masks", "npy"))}
    if refine:
        cached_path = os.path.join(root, "poses/anim_nerf_test.npz")
    elif os.path.exists(os.path.join(root, f"poses/anim_nerf_{split}.npz")):
        cached_path = os.path.join(root, f"poses/anim_nerf_{split}.npz")
    elif os.path.exists(os.path.join(root, f"poses/{split}.npz")):
        cached_path = os.path.join(root, f"poses/{split}.npz")
    else:
        cached_path = None
    cached = bool(cached_path and os.path.exists(cached_path))
    p = dict(np.load(cached_path if cached else os.path.join(root, "poses.npz")))
    if "thetas" in p:
        p["body_pose"], p["global_orient"] = p["thetas"][..., 3:], p["thetas"][..., :3]
    smpl = {k: p[k].astype(np.float32) for k in ("betas", "body_pose", "global_orient", "transl")}
    smpl["betas"] = smpl["betas"].reshape(1, 10)
    if not cached:
        smpl.update({k: smpl[k][sel] for k in ("body_pose", "global_orient", "transl")})
    F = len(lists["img_lists"])
    if near is not None and far is not None:
        near_tab, far_tab = np.ones(F, np.float32) * near, np.ones(F, np.float32) * far
    else:
        if rana:                                                    # distance from the camera at the origin to the mid-hip
            dist = [np.sqrt(np.square(smpl["transl"][i]).sum(-1)) for i in range(F)]
        else:
            camera_loc = RT[:3, :3].T @ -RT[:3, 3]
            dist = [np.sqrt(np.square(camera_loc - smpl["transl"][i]).sum(-1)) for i in range(F)]
        dist = np.array(dist, np.float32)
        near_tab, far_tab = dist - 1, dist + 1
    return dict(kind=kind, root=root, K=K, w2c=RT, c2w=c2w, height=height, width=width, full_height=full_height, full_width=full_width,
                img_wh=(width, height), downscale=s, hdri_files=hdri_files, near=near_tab.astype(np.float32), far=far_tab.astype(np.float32),
                dilate_k=TRUTH_KINDS[kind], **lists, **smpl)


def downscale_center(x: Tensor, s: int) -> Tensor:
    """cv2.resize(x, dsize=None, fx=1/s, fy=1/s) (default INTER_LINEAR) of every frame of x -- uint8 [F,H,W,C] or [F,H,W], or float32
    [F,H,W] -- for an even s that divides H and W: the centre 2 x 2 of every s x s block (csrc/data_math.h)."""
    if not x.is_cuda:
        raise L.IaError("intrinsicavatar_amd operators need GPU tensors (no CPU fallback)")
    if x.dim() not in (3, 4) or x.dtype not in (torch.uint8, torch.float32) or (x.dim() == 4 and x.dtype != torch.uint8):
        raise TypeError(f"downscale_center needs uint8 [F,H,W,C] / [F,H,W] or float32 [F,H,W], got {x.dtype} {tuple(x.shape)}")
    F, H, W = (int(v) for v in x.shape[:3])
    s = _center_factor(s, H, W)
    if s == 1:
        raise NotImplementedError("downscale_center needs a factor above 1")
    x = x.contiguous()
    out = torch.empty((F, H // s, W // s) + tuple(x.shape[3:]), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        if x.dtype == torch.uint8:
            ch = int(x.shape[3]) if x.dim() == 4 else 1
            L.lib().ia_downscale_center_u8(F, H, W, ch, s, x, out)
        else:
            L.lib().ia_downscale_center_f32(F, H, W, s, x, out)
    return out


def valid_rect(masks: Tensor, k: int) -> Tensor:
    """masks float32 [F,H,W] on the GPU -> (x, y, w, h) int32 [F,4] of cv2.boundingRect(cv2.dilate(msk.astype(np.uint8), ones(k, k))) of
    every frame, (0, 0, 0, 0) where no pixel counts (ia_truth_valid_rect)."""
    if not masks.is_cuda:
        raise L.IaError("intrinsicavatar_amd operators need GPU tensors (no CPU fallback)")
    if masks.dtype != torch.float32 or masks.dim() != 3:
        raise TypeError(f"valid_rect needs float32 [F,H,W], got {masks.dtype} {tuple(masks.shape)}")
    masks = masks.contiguous()
    F, H, W = (int(v) for v in masks.shape)
    rect = torch.empty((F, 4), dtype=torch.int32, device=masks.device)
    with torch.cuda.device(masks.device):
        L.lib().ia_truth_valid_rect(F, H, W, masks, int(k), rect)
    return rect


class TruthFrames(TrainingFrames):
    """TrainingFrames with ground truth: RANADataset / SyntheticHumanDataset on the device.  albedos, normals: uint8 [F,H,W,3] GPU tensors
    like images; w2c [4,4] (the extrinsic); valid_dilate: the side of the valid mask's dilate kernel; hdri_files: one path per frame (the
    test split); near_far: (near [F], far [F]) tables instead of the |transl| -+ 1 rule; img_wh: default (W, H)."""
    HDRI_RESIDENT = 2

    def __init__(self, images: Tensor, masks: Tensor, K, c2w, smpl_params: Dict, sampler=None, near=None, far=None, *, albedos: Tensor,
                 normals: Tensor, w2c, valid_dilate: int = 100, hdri_files=None, near_far=None, img_wh=None):
        super().__init__(images, masks, K, c2w, smpl_params, sampler, near, far)
        for name, t in (("albedos", albedos), ("normals", normals)):
            if not t.is_cuda:
                raise L.IaError("intrinsicavatar_amd operators need GPU tensors (no CPU fallback)")
            if t.dtype != torch.uint8 or t.shape != self.images.shape:
                raise TypeError(f"{name} must be uint8 {tuple(self.images.shape)} like images, got {t.dtype} {tuple(t.shape)}")
        self.albedos, self.normals = albedos.contiguous(), normals.contiguous()
        w2c = _host(w2c).astype(np.float32)
        if w2c.shape != (4, 4):
            raise ValueError(f"w2c must be [4,4], got {w2c.shape}")
        self.w2c = torch.from_numpy(np.ascontiguousarray(w2c)).to(self.device)[None]
        if hdri_files is not None and len(hdri_files) != self.F:
            raise ValueError(f"{len(hdri_files)} hdri_files for {self.F} frames")
        self.hdri_files = None if hdri_files is None else list(hdri_files)
        self._hdri = {}
        if near_far is not None:
            tabs = [np.ascontiguousarray(_host(t), dtype=np.float32).reshape(-1) for t in near_far]
            if any(t.shape != (self.F,) for t in tabs):
                raise ValueError(f"near_far needs two tables of {self.F} values")
            self.near, self.far = (torch.from_numpy(t).to(self.device) for t in tabs)
        self.img_wh = (self.W, self.H) if img_wh is None else tuple(img_wh)
        self.valid_dilate = int(valid_dilate)
        self.valid_rect = valid_rect(self.masks, self.valid_dilate)

    def _truth(self, out: Dict[str, Tensor], idx: int, n: int, pixels: Optional[Tensor]) -> Dict[str, Tensor]:
        dev = self.device
        out["albedo"] = torch.empty((1, n, 3), dtype=torch.float32, device=dev)
        out["normal"] = torch.empty((1, n, 3), dtype=torch.float32, device=dev)
        out["valid_mask"] = torch.empty((1, n), dtype=torch.bool, device=dev)
        with torch.cuda.device(dev):
            L.lib().ia_sample_truth(n, int(idx), self.F, self.H, self.W, pixels, self.albedos, self.normals, self.valid_rect, out["albedo"],
                                    out["normal"], out["valid_mask"])
        out["w2c"] = self.w2c
        return out

    def batch(self, idx: int, generator: Optional[torch.Generator] = None, words: Optional[Tensor] = None) -> Dict[str, Tensor]:
        """TrainingFrames.batch (the same call) + albedo, normal [1,n,3] float32, valid_mask bool at its pixel_indices and w2c [1,4,4]: the
        train datum of datasets/rana.py / synthetichuman.py.  One more kernel on the same stream, no host synchronisation.  valid_mask is
        [1,n,1] here, as the reference collates it (its sampler hands every extra array back as [n, -1]), and [1,n] from full_frame;
        preprocess_data flattens both."""
        out = super().batch(idx, generator, words)
        out = self._truth(out, idx, int(self.sampler.num_sample), out["pixel_indices"])
        out["valid_mask"] = out["valid_mask"][..., None]
        return out

    def full_frame(self, idx: int) -> Dict[str, Tensor]:
        """the test datum: every pixel in order, + hdri [1,h,w,3] float32 when the frames name their HDRIs."""
        out = self._truth(super().full_frame(idx), idx, self.H * self.W, None)
        if self.hdri_files is not None:
            out["hdri"] = self.hdri(self.hdri_files[int(idx)])
        return out

    def hdri(self, path: str) -> Tensor:
        """the environment map at `path` on the device, [1,h,w,3] float32 at its own size (the reference does not resize it); at most
        HDRI_RESIDENT maps stay resident, and frames that name one file share one tensor."""
        if path in self._hdri:
            self._hdri[path] = self._hdri.pop(path)                 # most recently used last
            return self._hdri[path]
        ext = os.path.splitext(path)[1].lower()
        if ext == ".exr":
            raise NotImplementedError("OpenEXR is not available in this image: convert the environment map to Radiance .hdr")
        from . import io_formats
        img = io_formats.load_hdr(path)
        while len(self._hdri) >= self.HDRI_RESIDENT:
            self._hdri.pop(next(iter(self._hdri)))
        self._hdri[path] = torch.from_numpy(np.ascontiguousarray(img, np.float32)).to(self.device)[None]
        return self._hdri[path]

    @classmethod
    def from_host(cls, host: Dict, sampler=None, near=None, far=None, device="cuda") -> "TruthFrames":
        """truth_host(...)'s files read once (PNGs through PIL, masks through np.load), moved to `device` at full resolution and, for
        downscale > 1, reduced there: images, albedos, normals as uint8, masks in the files' own type (uint8, or floating as float32) --
        cv2.resize works on what np.load returned, before msk.astype(np.float32)."""
        device = _need_gpu(device)
        from PIL import Image
        shape = (host["full_height"], host["full_width"])
        stacks = {}
        for name in ("img_lists", "albedo_lists", "normal_lists"):
            a = np.stack([np.asarray(Image.open(f).convert("RGB"), np.uint8) for f in host[name]])
            if a.shape[1:3] != shape:
                raise ValueError(f"{name[:-6]} files are {a.shape[1:3]}, cameras.json says {shape}")
            stacks[name] = torch.from_numpy(a).to(device)
        raw = [np.load(f) for f in host["msk_lists"]]
        if any(m.shape != shape for m in raw):
            raise ValueError(f"masks are {sorted({m.shape for m in raw})}, cameras.json says {shape}")
        s = host["downscale"]
        if s > 1 and all(m.dtype == np.uint8 for m in raw):
            masks = downscale_center(torch.from_numpy(np.stack(raw)).to(device), s).to(torch.float32)
        elif s > 1 and all(m.dtype.kind == "f" for m in raw):
            masks = downscale_center(torch.from_numpy(np.stack([m.astype(np.float32) for m in raw])).to(device), s)
        elif s > 1:
            raise NotImplementedError(f"downscale of masks of type {sorted({str(m.dtype) for m in raw})}: uint8 or floating point, not mixed")
        else:
            masks = torch.from_numpy(np.stack([m.astype(np.float32) for m in raw])).to(device)
        if s > 1:
            stacks = {k: downscale_center(v, s) for k, v in stacks.items()}
        # (an optimised pose file is not sliced by the reference: frame idx reads its row idx, the rows past the frame list are never read)
        smpl = {k: host[k] if k == "betas" else host[k][:len(raw)] for k in ("betas", "body_pose", "global_orient", "transl")}
        explicit = near is not None and far is not None
        return cls(stacks["img_lists"], masks, host["K"], host["c2w"], smpl, sampler, near if explicit else None, far if explicit else None,
                   albedos=stacks["albedo_lists"], normals=stacks["normal_lists"], w2c=host["w2c"], valid_dilate=host["dilate_k"],
                   hdri_files=host["hdri_files"], near_far=None if explicit else (host["near"], host["far"]), img_wh=host["img_wh"])

    @classmethod
    def from_rana(cls, data_root: str, subject: str, split: str, start: int, end: int, skip: int = 1, sampler=None, near=None, far=None,
                  refine: bool = False, downscale=1, device="cuda") -> "TruthFrames":
        """RANADataset (datasets/rana.py): data_root/split/subject with cameras.json, images/, albedos/, normals/, masks/, poses."""
        device = _need_gpu(device)
        return cls.from_host(truth_host("rana", data_root, subject, split, start, end, skip, downscale, near, far, refine), sampler, near, far,
                             device)

    @classmethod
    def from_synthetichuman(cls, data_root: str, subject: str, split: str, start: int, end: int, skip: int = 1, sampler=None, near=None,
                            far=None, refine: bool = False, downscale=1, device="cuda") -> "TruthFrames":
        """SyntheticHumanDataset (datasets/synthetichuman.py): data_root/subject, camera "00" of cameras.json, images/00 (images_relit/00 on
        the test split), albedos_png/00, normals_png/00, masks/00."""
        device = _need_gpu(device)
        return cls.from_host(truth_host("synthetichuman", data_root, subject, split, start, end, skip, downscale, near, far, refine), sampler,
                             near, far, device)
