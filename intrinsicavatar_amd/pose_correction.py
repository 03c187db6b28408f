"""Per-frame corrections of the SMPL fits (models/pose/pose_correction.py): four zero-initialised embeddings under the reference's
names, switched on by the step counter.  fit.Trainer adds them to the dataset's parameters before the kinematics; the gradient
reaches them through smpl.SMPLKinematics, smpl.deformer_transforms and the deformer's pose terms (deformer._PoseTerms).

state_dict keys (= the reference's, under `model.pose_correction.` in a checkpoint):
    pose_correction.weight [F,69], shape_correction.weight [1,10], global_orient_correction.weight [F,3], transl_correction.weight [F,3]
"""
from typing import Dict

import torch
from torch import Tensor


class PoseCorrection(torch.nn.Module):
    def __init__(self, dataset_length: int, enable_pose_correction: bool = False, pose_correction_start_step: int = 4000):
        super().__init__()
        self.dataset_length = int(dataset_length)
        self.config_enable_pose_correction = bool(enable_pose_correction)          # config.enable_pose_correction of the reference
        self.pose_correction_start_step = int(pose_correction_start_step)
        self.pose_correction = torch.nn.Embedding(self.dataset_length, 69)
        self.shape_correction = torch.nn.Embedding(1, 10)
        self.global_orient_correction = torch.nn.Embedding(self.dataset_length, 3)
        self.transl_correction = torch.nn.Embedding(self.dataset_length, 3)
        with torch.no_grad():
            for emb in (self.pose_correction, self.shape_correction, self.global_orient_correction, self.transl_correction):
                emb.weight.zero_()
        self.enable_pose_correction = False          # the switch: update_step turns it on, nothing turns it off

    def forward(self, idx: Tensor) -> Dict[str, Tensor]:
        """idx: int64 frame indices [n] -> the four corrections; while the switch is off, zeros of shape [1, .] whatever idx is.
        The shape row does not depend on idx."""
        if self.enable_pose_correction:
            betas = self.shape_correction(torch.zeros(1, device=idx.device).long())
            orient = self.global_orient_correction(idx)
            transl = self.transl_correction(idx)
            pose = self.pose_correction(idx)
        else:
            betas = torch.zeros_like(self.shape_correction.weight)
            orient = torch.zeros_like(self.global_orient_correction.weight[:1])
            transl = torch.zeros_like(self.transl_correction.weight[:1])
            pose = torch.zeros_like(self.pose_correction.weight[:1])
        return dict(betas_correction=betas, global_orient_correction=orient, transl_correction=transl, pose_correction=pose)

    def update_step(self, epoch: int, global_step: int) -> None:
        if self.config_enable_pose_correction and global_step > self.pose_correction_start_step:
            self.enable_pose_correction = True
