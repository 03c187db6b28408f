"""Drop-in for the part of `lib.pytorch3d.ops` the reference uses (models/deformers/fast_snarf/deformer_torch.py:1 and :236):

    knn_points(p1, p2, K=...)   -> lib/pytorch3d/ops/knn.py; values as its CPU implementation lib/pytorch3d/cuda/knn_cpu.cpp:13-69
    knn_gather(x, idx)

Forward only (the reference calls it on detached tensors); brute force on the GPU (csrc/skinning.hip, ia_knn_points).  Squared distances
((dx*dx + dy*dy) + dz*dz in float32), the K smallest pairs under the order (distance, index), ascending: equal distances are ordered by
index, whatever the launch."""
from collections import namedtuple
from typing import Optional

import torch
from torch import Tensor

from . import _lib as L

_KNN = namedtuple("KNN", "dists idx knn")
MAX_K = 32


def knn_points_flat(p1: Tensor, p2: Tensor, K: int):
    """p1 [P,3], p2 [V,3] fp32 on the GPU -> (d2 [P,K] fp32, idx [P,K] int32)."""
    P, V = p1.shape[0], p2.shape[0]
    d2 = torch.empty((P, K), dtype=torch.float32, device=p1.device)
    idx = torch.empty((P, K), dtype=torch.int32, device=p1.device)
    L.lib().ia_knn_points(P, V, K, p1, p2, d2, idx)
    return d2, idx


def _full_lengths(lengths: Optional[Tensor], n: int, name: str):
    if lengths is not None and not bool((lengths == n).all()):
        raise NotImplementedError(f"knn_points: ragged {name} (every cloud must have its full length)")


def knn_points(p1: Tensor, p2: Tensor, lengths1: Optional[Tensor] = None, lengths2: Optional[Tensor] = None, norm: int = 2, K: int = 1,
               version: int = -1, return_nn: bool = False, return_sorted: bool = True):
    """p1 [N,P1,3], p2 [N,P2,3] -> KNN(dists [N,P1,K] squared, idx [N,P1,K] int64, knn [N,P1,K,3] or None).  `version` selects among
    pytorch3d's CUDA kernels and changes nothing here; the result is always sorted."""
    if p1.dim() != 3 or p2.dim() != 3 or p1.shape[0] != p2.shape[0]:
        raise ValueError("knn_points: p1 [N,P1,D] and p2 [N,P2,D] with one batch size")
    if p1.shape[2] != 3 or p2.shape[2] != 3:
        raise NotImplementedError("knn_points: D != 3")
    if norm != 2:
        raise NotImplementedError("knn_points: norm != 2")
    if not 1 <= K <= MAX_K:
        raise NotImplementedError(f"knn_points: K > {MAX_K} (or K < 1)")
    if p2.shape[1] < K:
        raise NotImplementedError("knn_points: K larger than the number of points in p2")
    if p1.requires_grad or p2.requires_grad:
        raise NotImplementedError("knn_points: forward only (requires_grad: detach the inputs, as the reference does)")
    _full_lengths(lengths1, p1.shape[1], "lengths1")
    _full_lengths(lengths2, p2.shape[1], "lengths2")
    if not (p1.is_cuda and p2.is_cuda):
        raise L.IaError("knn_points needs GPU tensors (no CPU fallback)")
    p1, p2 = p1.contiguous().float(), p2.contiguous().float()
    outs = [knn_points_flat(p1[n], p2[n], K) for n in range(p1.shape[0])]
    dists = torch.stack([o[0] for o in outs])
    idx = torch.stack([o[1] for o in outs]).long()
    return _KNN(dists, idx, knn_gather(p2, idx) if return_nn else None)


def knn_gather(x: Tensor, idx: Tensor, lengths: Optional[Tensor] = None) -> Tensor:
    """x [N,M,U], idx [N,L,K] -> [N,L,K,U] (lib/pytorch3d/ops/knn.py knn_gather; no padding: every cloud has its full length)."""
    N, M, U = x.shape
    _full_lengths(lengths, M, "lengths")
    _, Lq, K = idx.shape
    return x[:, :, None].expand(-1, -1, K, -1).gather(1, idx[:, :, :, None].expand(-1, -1, -1, U))
