"""Plain numpy / scipy restatement of the reference's LSD error maps (the test-side model of the LSD form of
bootstrapper_amd/evaluate.py), in the reference's calls, order and dtypes:

  compute_errors (eval/compute_errors.py:25-223): gp.Pad(seg, context), gp.Pad(pred, None), gp.Pad(mask, None) ->
  gp.Normalize(pred) -> AddLSDErrors (gp/add_lsd_errors.py: LsdExtractor.get_descriptors, _create_diff, _create_mask) ->
  IntensityScaleShift(255) -> AsType(uint8), chunk by chunk in gp.Scan's order.

Every chunk is processed over the region the reference requests for SEG_PRED: the chunk grown by `margin` voxels per side
((2, 50, 50) there: input_shape - output_shape = (4, 100, 100)).  Descriptors, the normalising maximum and the morphology
are taken over that grown region, and the chunk is cropped out of it at the end.

The lsd package is not installed here: oracle/lsd_ref.py restates get_descriptors (parity unpinned).  skimage is absent
too: ball(1)[0] and disk(1) are written out.  tools/gen_goldens_eval_lsd.py pins this file where gunpowder and lsd import."""
import numpy as np
from scipy.ndimage import binary_dilation, binary_erosion

from eval_ref import padded, scan_chunks
from oracle.lsd_ref import lsd_targets

# np.stack([ball(1)[0]] * 3): ball(1)[0] is the 3 x 3 plane with only its centre set, so this is the 3 x 1 x 1 column
Z_STRUCT = np.zeros((3, 3, 3), bool)
Z_STRUCT[:, 1, 1] = True
# np.stack([zeros((3, 3)), disk(1), zeros((3, 3))]): the in-plane 4-neighbour cross
XY_STRUCT = np.zeros((3, 3, 3), bool)
XY_STRUCT[1] = [[0, 1, 0], [1, 1, 1], [0, 1, 0]]

MARGIN = (2, 50, 50)
DOWNSAMPLE = 2


def default_sigma(voxel_size):
    return int(voxel_size[-1] * 10)


def context_voxels(sigma, voxel_size):
    """3 sigma in world units around a voxel-aligned ROI, snapped to the voxel grid by shrinking"""
    return [int(np.floor(3 * sigma / v)) for v in voxel_size]


def create_diff(a, b, mask=None):
    """AddLSDErrors._create_diff -> (normalised diff, diff before normalisation, the maximum)"""
    diff = np.sum((a - b) ** 2, axis=0)
    if mask is not None:
        diff *= mask
    raw = diff.copy()
    m = np.max(diff)
    if m > 0:
        diff /= m
    else:
        diff[:] = 0
    return diff, raw, m


def threshold(d, thresholds):
    floor, ceil = thresholds
    return (d > floor) & (d < ceil)


def morphology(o):
    """the morphology of AddLSDErrors._create_mask on the thresholded mask (bool), scipy's border_value = 0 throughout"""
    o = binary_erosion(o, XY_STRUCT, iterations=4)
    o = binary_dilation(o, XY_STRUCT, iterations=4)
    o = binary_dilation(o, Z_STRUCT)
    o = binary_erosion(o, Z_STRUCT)
    return o.astype(np.uint8)


def diamond(radius):
    """the in-plane L1 ball as a 1 x (2r+1) x (2r+1) structuring element"""
    y, x = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    return (np.abs(y) + np.abs(x) <= radius)[None]


def morphology_one_pass(o):
    """the same mask by one erosion and one dilation with the diamond of radius 4, and one z closing"""
    o = binary_erosion(o, diamond(4))
    o = binary_dilation(o, diamond(4))
    o = binary_dilation(o, Z_STRUCT)
    return binary_erosion(o, Z_STRUCT).astype(np.uint8)


def lsd_errors(seg, seg_begin, pred, pred_begin, roi_shape, chunk, sigma, voxel_size, thresholds=(0.1, 1.0), mask=None,
               mask_begin=None, margin=MARGIN, downsample=DOWNSAMPLE, stages=None):
    """error_map, error_mask (u8, ROI-shaped).  seg, pred ([10][...] u8), mask: whole datasets; *_begin: the ROI's first
    voxel in each dataset's index space.  stages: a list that receives, per chunk in Scan's order, a dict of the chunk's
    origin and its intermediate arrays over the grown region (desc, pred, diff, max, raw)."""
    chunk = [min(c, n) for c, n in zip(chunk, roi_shape)]
    ctx = context_voxels(sigma, voxel_size)
    grown = [c + 2 * m for c, m in zip(chunk, margin)]
    factor = np.float32(1.0 / 255)
    emap = np.zeros(roi_shape, np.uint8)
    emask = np.zeros(roi_shape, np.uint8)
    crop = tuple(slice(m, m + c) for m, c in zip(margin, chunk))
    for org in scan_chunks(roi_shape, chunk):
        g0 = [o - m for o, m in zip(org, margin)]   # the grown region's first voxel, ROI coordinates
        labels = padded(seg, [b + g - k for b, g, k in zip(seg_begin, g0, ctx)], [g + 2 * k for g, k in zip(grown, ctx)])
        desc = lsd_targets(labels, ctx, grown, [float(sigma)] * 3, voxel_size, downsample)[0]
        p = np.stack([padded(pred[c], [b + g for b, g in zip(pred_begin, g0)], grown) for c in range(pred.shape[0])])
        p = p.astype(np.float32) * factor
        mk = None if mask is None else padded(mask, [b + g for b, g in zip(mask_begin, g0)], grown)
        d, raw_diff, m = create_diff(desc, p, mk)
        raw = threshold(d, thresholds)
        closed = morphology(raw)
        sl = tuple(slice(o, o + c) for o, c in zip(org, chunk))
        emask[sl] = closed[crop]
        emap[sl] = (d[crop] * 255 + 0).astype(np.uint8)
        if stages is not None:
            stages.append({"origin": tuple(org), "desc": desc, "pred": p, "diff": raw_diff, "max": m, "raw": raw.astype(np.uint8)})
    return emap, emask


def direct_descriptor(labels, p, sigma, voxel_size, downsample):
    """the 10 descriptors of voxel p of `labels` (int [D][H][W], the whole label array) by the device kernel's formula, in
    float64: a direct sum over the window of p's cell on the sub-grid labels[::df], coordinates relative to the cell, weights
    as scipy's gaussian_filter1d builds them; a label that no tap holds takes the library's count-of-1 branch (absolute mean
    0, covariance 0).  float64 [10], before the cast to float32."""
    df = int(downsample)
    l = labels[tuple(p)]
    if l == 0:
        return np.zeros(10)
    sub = labels[::df, ::df, ::df]
    cell = [int(x) // df for x in p]
    sigma = np.asarray(sigma, np.float64)
    step = np.asarray(voxel_size, np.float64) * df
    w, c = [], []
    for d in range(3):
        sv = sigma[d] / step[d]
        r = int(3.0 * sv + 0.5)
        k = np.arange(-r, r + 1)
        g = np.exp(-0.5 * k.astype(np.float64) ** 2 / (sv * sv))
        g /= g.sum()
        inside = (cell[d] + k >= 0) & (cell[d] + k < sub.shape[d])
        w.append((g[inside], k[inside]))
        c.append(k[inside] * step[d])
    win = sub[np.ix_(*[cell[d] + w[d][1] for d in range(3)])] == l
    wgt = w[0][0][:, None, None] * w[1][0][None, :, None] * w[2][0][None, None, :] * win
    cz, cy, cx = c[0][:, None, None], c[1][None, :, None], c[2][None, None, :]
    n = wgt.sum()
    if n == 0:
        mean = -np.asarray(cell, np.float64) * step
        var, pe = np.zeros(3), np.zeros(3)
    else:
        mean = np.array([(wgt * cz).sum(), (wgt * cy).sum(), (wgt * cx).sum()]) / n
        var = np.array([(wgt * cz * cz).sum(), (wgt * cy * cy).sum(), (wgt * cx * cx).sum()]) / n - mean * mean
        pe = np.array([(wgt * cz * cy).sum(), (wgt * cz * cx).sum(), (wgt * cy * cx).sum()]) / n
        pe -= np.array([mean[0] * mean[1], mean[0] * mean[2], mean[1] * mean[2]])
    var = np.maximum(var, 1e-3)
    pe = pe / np.sqrt(np.array([var[0] * var[1], var[0] * var[2], var[1] * var[2]]))
    out = np.concatenate([mean / sigma * 0.5 + 0.5, var / sigma ** 2, pe * 0.5 + 0.5, [n]])
    return np.clip(out, 0.0, 1.0)
