"""Geometric augmentation of the synthetic labels of the second-stage setups on the device: the SimpleAugment -> DeformAugment ->
ShiftAugment that models/3d_affs_from_2d_mtlsd/train.py:80-91 and its three siblings put directly behind CreateLabels +
gp.Pad(labels, None), before CustomGrowBoundary, ObfuscateLabels, the input arrays and the targets.  The three nodes are the one
coordinate map s(p) of augment.py (csrc/augment.hip: bsmi_aug_coords, then bsmi_aug_sample_nearest_i64), taken of
the created block itself; what this module adds is the rule for a voxel whose source lies outside the block (section 7o):

    labels are 0 outside the block (gp.Pad(labels, None)), never the replicated border.

Specified in the frame of the block padded by one voxel of zeros on every side, I = the block's shape, c = (I - 1) / 2:

    s'(p) = the coordinates of bsmi_aug_coords with src_centre = c + 1 (box_lo = (-1, -1, -1))
    q_a   = floor(s'_a + 1/2) - 1, the sum and the floor in float32
    out   = labels[q] if 0 <= q_a < I_a on all three axes, else 0

which is exactly the nearest sampling of the zero-padded block: an index the launch clamps lands on the zero border, and so does
NaN (index 0).  No new kernel and no new entry point: one torch pad and the two launches that are there.

These are specified rules, not a transcription of gunpowder, which is not installed where this was written: parity with the
reference is in distribution.  Declared difference: the labels are always created at input_shape and then warped; the reference
creates the intersection of the request, grown by the augmentations, with the block.
"""
import dataclasses

import numpy as np

from . import augment
from .augment import AugParams

SPACING_VOXELS = (4.0, 10.0, 10.0)   # control_point_spacing = voxel_size * (4, 10, 10) at the call sites
JITTER_VOXELS = (1.0, 2.0, 2.0)      # jitter_sigma = voxel_size * (1, 2, 2)


@dataclasses.dataclass(frozen=True)
class LabelAugParams:
    """The arguments of the three nodes, fields and units those of `[augment]` (augment.AugParams) without `intensity`; the
    defaults are the second-stage call sites' (models/3d_affs_from_2d_mtlsd/train.py:80-91).  deform_p: the call passes no p,
    so the node always applies.  control_point_spacing / jitter_sigma: world units per axis, None = voxel_size * (4, 10, 10)
    and voxel_size * (1, 2, 2), i.e. 4 / 10 / 10 and 1 / 2 / 2 voxels at any voxel size.  rotate: about z (rotation_axes=[1, 2])."""
    simple: bool = True
    deform_p: float = 1.0
    scale_interval: tuple = (0.8, 1.2)
    rotate: bool = True
    control_point_spacing: tuple = None
    jitter_sigma: tuple = None
    shift_p: float = 0.8
    prob_slip: float = 0.1
    prob_shift: float = 0.1
    shift_sigma: float = 3.0

    @classmethod
    def from_config(cls, value, key="label_augment"):
        """The train TOML key `label_augment`: absent / false -> None (today's path), true -> the defaults, a table -> overrides."""
        if value is None or value is False:
            return None
        if value is True:
            return cls()
        if not isinstance(value, dict):
            raise ValueError(f"{key} must be true, false or a table, not {value!r}")
        names = [f.name for f in dataclasses.fields(cls)]
        unknown = sorted(set(value) - set(names))
        if unknown:
            raise ValueError(f"unknown {key} key(s) {', '.join(unknown)}; known: {', '.join(names)}")
        kw = {}
        for k, v in value.items():
            try:
                if k in ("simple", "rotate"):
                    if not isinstance(v, bool):
                        raise ValueError
                    kw[k] = v
                    continue
                if k in ("scale_interval", "control_point_spacing", "jitter_sigma"):
                    kw[k] = tuple(float(x) for x in v)
                else:
                    if isinstance(v, bool):
                        raise ValueError
                    kw[k] = float(v)
            except (TypeError, ValueError):
                what = ("true or false" if k in ("simple", "rotate") else "two numbers" if k == "scale_interval" else
                        "three world-unit values (z, y, x)" if k in ("control_point_spacing", "jitter_sigma") else "a number")
                raise ValueError(f"{key}.{k} {v!r}: {what}") from None
            if k == "scale_interval":
                if len(kw[k]) != 2 or not 0 < kw[k][0] <= kw[k][1]:
                    raise ValueError(f"{key}.scale_interval {v!r}: two positive numbers, low <= high")
            elif k in ("control_point_spacing", "jitter_sigma"):
                if len(kw[k]) != 3 or (k == "control_point_spacing" and min(kw[k]) <= 0) or min(kw[k]) < 0:
                    raise ValueError(f"{key}.{k} {v!r}: three world-unit values (z, y, x)")
            elif kw[k] < 0 or (k != "shift_sigma" and kw[k] > 1):
                raise ValueError(f"{key}.{k} {v!r}: " + ("not negative" if k == "shift_sigma" else "a probability"))
        return cls(**kw)

    def spacing(self, voxel_size):
        """control_point_spacing in world units at `voxel_size`"""
        return self.control_point_spacing or tuple(float(v) * s for v, s in zip(voxel_size, SPACING_VOXELS))

    def to_aug_params(self, voxel_size):
        """The augment.AugParams that augment.draw_plan takes, spacing and jitter spelled out at `voxel_size`: the draws and
        their order are draw_plan's documented ones."""
        jitter = self.jitter_sigma or tuple(float(v) * s for v, s in zip(voxel_size, JITTER_VOXELS))
        return AugParams(simple=self.simple, deform_p=self.deform_p, scale_interval=self.scale_interval, rotate=self.rotate,
                         control_point_spacing=tuple(self.spacing(voxel_size)), jitter_sigma=tuple(jitter), shift_p=self.shift_p,
                         prob_slip=self.prob_slip, prob_shift=self.prob_shift, shift_sigma=self.shift_sigma, intensity=None)


def check_block(params, shape, voxel_size, key="label_augment"):
    """What no plan of `params` for a block of `shape` could be drawn or launched with, refused by the name of the key to
    change: a y/x swap of a non-square block, a rotation about z on an anisotropic section grid, a control lattice of more
    nodes than the coordinate launch holds.  Touches no GPU.  Returns the lattice's nodes per axis (None without DeformAugment)."""
    shape = tuple(int(v) for v in shape)
    vs = [float(v) for v in voxel_size]
    if params.simple:
        augment.check_square(shape, shape, key)
    if params.deform_p <= 0:
        return None
    if params.rotate and vs[1] != vs[2]:
        raise NotImplementedError(f"rotation about z needs voxel_size[1] == voxel_size[2], not {vs}; set {key}.rotate = false "
                                  "(full 3-D rotations are not built)")
    spacing = [c / v for c, v in zip(params.spacing(vs), vs)]
    n = augment.lattice_shape(shape, spacing)
    if n[0] * n[1] * n[2] > augment.MAX_LATTICE_NODES:
        raise ValueError(f"control lattice of {n} nodes for a block of {list(shape)} at spacing {spacing} voxels: at most "
                         f"{augment.MAX_LATTICE_NODES}; raise {key}.control_point_spacing")
    return n


def is_identity(plan):
    """no mirror, swap, lattice or shifts, and linear = (1, 1, 0, 0, 1): the map is s(p) = p"""
    return (not any(plan.mirror) and not plan.swap and plan.lattice is None and plan.shifts is None
            and np.array_equal(np.asarray(plan.linear, dtype=np.float32), np.array([1, 1, 0, 0, 1], dtype=np.float32)))


def warp_labels(labels, plan):
    """labels (int64 CUDA (D, H, W), contiguous, of plan.shape) through the map of `plan` (an augment.AugPlan), 0 where the
    source lies outside the block: the block padded by one voxel of zeros, augment.coords with box_lo = (-1, -1, -1),
    augment.sample_labels.  On torch's current stream.  An identity plan returns `labels` itself, without a launch."""
    import torch
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.dim() != 3 or not labels.is_cuda or not labels.is_contiguous():
        raise ValueError("labels must be a contiguous int64 CUDA tensor (D, H, W)")
    if tuple(labels.shape) != tuple(plan.shape):
        raise ValueError(f"labels of shape {tuple(labels.shape)} for a plan of {tuple(plan.shape)}")
    if is_identity(plan):
        return labels
    padded = torch.nn.functional.pad(labels, (1, 1, 1, 1, 1, 1)).contiguous()
    return augment.sample_labels(augment.coords(plan, (-1, -1, -1), labels.device), padded)
