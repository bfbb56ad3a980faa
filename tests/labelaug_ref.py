"""numpy statement of the rule of bootstrapper_amd/augment_labels.py for the tests: synthetic labels warped
through the coordinate map of augment.py are 0 where the source lies outside the block.  The coordinates s' are GIVEN (the device's
read-back planes, or aug_ref.emulate_coords), in the frame of the block padded by one voxel: box_lo = (-1, -1, -1).

rule()     the rule as written, without padding: q_a = floor(s'_a + 1/2) - 1, the sum and the floor in float32; labels[q] where
           0 <= q_a < I_a on all three axes, else 0.  NaN compares false and gives 0.
padded()   what the device does: aug_ref.sample_nearest of the block padded by one voxel of zeros.
clamping() the fault to be refused: the same indices clamped to the block itself, which replicates the border labels outwards.
"""
import numpy as np

import aug_ref as R

BOX_LO = (-1, -1, -1)


def rule(coords, labels):
    s = np.asarray(coords, dtype=np.float32)
    inside = np.ones(s.shape[1:], dtype=bool)
    q = []
    for a in range(3):
        v = np.floor(s[a] + np.float32(0.5)) - np.float32(1.0)
        ok = (v >= 0) & (v < labels.shape[a])
        inside &= ok
        q.append(np.where(ok, v, np.float32(0.0)).astype(np.int64))
    return np.where(inside, labels[q[0], q[1], q[2]], 0).astype(labels.dtype)


def padded(coords, labels):
    return R.sample_nearest(coords, np.pad(labels, 1))


def clamping(coords, labels):
    return R.sample_nearest(np.asarray(coords, dtype=np.float32) - np.float32(1.0), labels)


def zero_share(coords, shape):
    """the share of voxels whose source lies outside a block of `shape`"""
    return float((rule(coords, np.ones(shape, dtype=np.int64)) == 0).mean())


def mild_plan(shape):
    """u = 1.2, theta = 0, no lattice, no shifts: the block shrinks about its centre and a frame of zeros enters"""
    from bootstrapper_amd.augment import AugPlan
    return AugPlan(shape, u=1.2, theta=0.0)


def shifted_expected(labels, shifts):
    """an integer-shift-only plan: section z is labels[z] moved by (sh_y, sh_x), zeros entering"""
    d, h, w = labels.shape
    out = np.zeros_like(labels)
    for z in range(d):
        sy, sx = int(shifts[0, z]), int(shifts[1, z])
        y0, y1 = max(0, -sy), min(h, h - sy)
        x0, x1 = max(0, -sx), min(w, w - sx)
        if y1 > y0 and x1 > x0:
            out[z, y0:y1, x0:x1] = labels[z, y0 + sy:y1 + sy, x0 + sx:x1 + sx]
    return out
