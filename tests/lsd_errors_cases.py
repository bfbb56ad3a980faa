"""Inputs of the LSD error-map tests (tests/test_evaluate_lsd_cpu.py, tests/test_evaluate_lsd_gpu.py): a segmentation with
smoothed-noise blobs and a straight boundary, one-voxel objects and one-voxel-thick sheets (clamped variances; where they
fall between the sub-grid's points, windows without a single tap), ids above 2^32; and a pred dataset that holds the u8
descriptors of a different segmentation (two objects merged, one split in z), so that the error map, the thresholded mask
and the morphology all have something to do."""
import numpy as np
from scipy.ndimage import gaussian_filter

from eval_ref import padded
from oracle.lsd_ref import lsd_targets

BIG = {3: 2**32 + 5, 9: 2**63 + 1, 11: 2**64 - 1}
THIN = {"voxels": 60, "sheet_z": 61, "sheet_y": 62}


def make_labels(rng, shape, roi_begin, roi_shape):
    """-> (labels u64, {name: voxels (n, 3) of the thin objects inside the ROI})"""
    blobs = gaussian_filter(rng.random(shape), (1, 4, 4))
    labels = (np.digitize(blobs, np.quantile(blobs, [0.2, 0.4, 0.6, 0.8])) + 1).astype(np.uint64)   # 1..5
    labels[:, :, shape[2] // 2:] += np.uint64(7)              # more objects, a straight boundary
    labels[blobs < np.quantile(blobs, 0.1)] = 0               # background
    b, s = roi_begin, roi_shape
    labels[b[0] + s[0] // 2, b[1] + 4:b[1] + s[1] - 4, b[2] + 3:b[2] + s[2] // 2] = THIN["sheet_z"]       # z-thin sheet
    labels[b[0] + 1:b[0] + s[0] - 1, b[1] + s[1] // 2 + 1, b[2] + s[2] // 2:b[2] + s[2] - 3] = THIN["sheet_y"]  # y-thin sheet
    for k in range(6):                                        # single voxels of one id, both parities on every axis
        labels[b[0] + 1 + k, b[1] + 2 + 3 * k, b[2] + 5 + 5 * k] = THIN["voxels"]
    for small, big in BIG.items():
        labels[labels == small] = np.uint64(big)
    roi = tuple(slice(o, o + n) for o, n in zip(b, s))
    thin = {name: np.argwhere(labels[roi] == v) + np.asarray(b) for name, v in THIN.items()}
    return labels, thin


def other_segmentation(labels):
    """two objects merged, one split in z"""
    out = labels.copy()
    out[out == 2] = 1
    z = out.shape[0] // 2
    out[z:][out[z:] == 4] = 40
    out[z:][out[z:] == 8] = 80
    return out


def u8_descriptors(labels, begin, shape, sigma, voxel_size, downsample, context):
    """the pred dataset a network would write for `labels`: descriptors over [begin, begin + shape) as u8"""
    df = downsample
    lo = [b - k - (b - k) % df for b, k in zip(begin, context)]                    # an even-aligned label array around the region
    hi = [b + n + k + (-(b + n + k)) % df for b, n, k in zip(begin, shape, context)]
    arr = padded(labels, lo, [h - l for l, h in zip(lo, hi)])
    off = [b - l for b, l in zip(begin, lo)]
    even = [n + (o % df) + (-(n + o % df)) % df for n, o in zip(shape, off)]        # ROI snapped outwards to the sub-grid
    off0 = [o - o % df for o in off]
    d = lsd_targets(arr, off0, even, [float(sigma)] * 3, voxel_size, df)[0]
    d = d[(slice(None),) + tuple(slice(o - o0, o - o0 + n) for o, o0, n in zip(off, off0, shape))]
    return (d * 255).astype(np.uint8)


def make_case(seed, voxel_size, sigma, downsample, roi_shape, margin, context, seg_begin=(3, 10, 12), pred_begin=(1, 3, 6),
              pred_after=(2, 6, 4), mask_begin=(2, 6, 2), with_mask=True, mask_max=1):
    """datasets around a ROI: seg holds the whole halo after the ROI and a part of it before; pred and mask hold a part of the
    margin on either side.  *_begin: the ROI's first voxel in each dataset."""
    rng = np.random.default_rng(seed)
    halo = [m + k for m, k in zip(margin, context)]
    seg_shape = [b + n + h for b, n, h in zip(seg_begin, roi_shape, halo)]
    seg, thin = make_labels(rng, seg_shape, seg_begin, roi_shape)
    pred_shape = [b + n + a for b, n, a in zip(pred_begin, roi_shape, pred_after)]
    pred = u8_descriptors(other_segmentation(seg), [s - p for s, p in zip(seg_begin, pred_begin)], pred_shape, sigma, voxel_size,
                          downsample, context)
    mask = None
    if with_mask:
        mask_shape = [b + n + 3 for b, n in zip(mask_begin, roi_shape)]
        mask = (rng.random(mask_shape) < 0.9).astype(np.uint8)
        mask[:, :2] = mask_max      # any u8 value multiplies
    return {"seg": seg, "seg_begin": list(seg_begin), "pred": pred, "pred_begin": list(pred_begin), "mask": mask,
            "mask_begin": list(mask_begin), "roi_shape": list(roi_shape), "thin": thin, "voxel_size": list(voxel_size),
            "sigma": sigma, "downsample": downsample, "margin": list(margin), "context": list(context)}
