"""Plain-numpy restatement of the reference's evaluation (the test-side model of bootstrapper_amd/evaluate.py, like
agglo_model.py is of the agglomeration).  It follows the reference's calls in their order and dtypes:

  compute_errors (eval/compute_errors.py:25-223): gp.Pad(seg, context) -> gp.Normalize(pred) -> AddAffErrors
  (gp/add_aff_errors.py: seg_to_affgraph, _create_diff, _create_mask) -> IntensityScaleShift(255) -> AsType(uint8),
  chunk by chunk in gp.Scan's order (z counted fastest, the last chunk of an axis moved back to end at the ROI's end);
  compute_stats (:226-239); funlib.evaluate.rand_voi on the masked volumes (eval/compute_metrics.py:104-110).

gunpowder's `seg_to_affgraph`, gp.Scan and funlib.evaluate are not installed here: they are restated, and
tools/gen_goldens_eval.py pins them where they are.  The normalising maximum is taken over the Scan chunk."""
import numpy as np

DEFAULT_NEIGHBORHOOD = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0], [0, 8, 0], [0, 0, 8]]


def seg_to_affgraph(seg, nhood):
    """gunpowder.nodes.add_affinities.seg_to_affgraph, 3-D: aff[e][v] = seg[v] == seg[v + o_e] and both are non-zero;
    0 where v + o_e leaves the array.  int32."""
    nhood = np.asarray(nhood)
    shape = seg.shape
    aff = np.zeros((nhood.shape[0],) + shape, dtype=np.int32)
    for e in range(nhood.shape[0]):
        o = nhood[e]
        dst = tuple(slice(max(0, -o[d]), min(shape[d], shape[d] - o[d])) for d in range(3))
        src = tuple(slice(max(0, o[d]), min(shape[d], shape[d] + o[d])) for d in range(3))
        aff[(e,) + dst] = (seg[dst] == seg[src]) * (seg[dst] > 0) * (seg[src] > 0)
    return aff


def scan_origins(n, c):
    """gp.Scan's chunk origins along one axis of extent n, chunk c (clamped to n): a grid from 0 with stride c whose last
    chunk is moved back to end at n"""
    c = min(c, n)
    out = list(range(0, n - c, c)) + [n - c]
    return out


def scan_chunks(roi_shape, chunk):
    """chunk origins in Scan's order: z counted fastest"""
    oz, oy, ox = (scan_origins(n, c) for n, c in zip(roi_shape, chunk))
    return [(z, y, x) for x in ox for y in oy for z in oz]


def padded(seg, begin, shape):
    """seg[begin : begin + shape] with zeros beyond the array (gp.Pad)"""
    out = np.zeros(shape, dtype=seg.dtype)
    lo = [max(0, b) for b in begin]
    hi = [min(n, b + s) for n, b, s in zip(seg.shape, begin, shape)]
    if all(h > l for l, h in zip(lo, hi)):
        out[tuple(slice(l - b, h - b) for l, h, b in zip(lo, hi, begin))] = seg[tuple(slice(l, h) for l, h in zip(lo, hi))]
    return out


def aff_errors(seg, roi_begin, pred, nhood, chunk, thresholds=(0.1, 1.0), mask=None):
    """error_map, error_mask (u8, ROI-shaped) of the affinity form.  seg: the whole seg dataset (any int dtype);
    roi_begin: the ROI's first voxel in seg's index space; pred: u8 [K][ROI]; mask: [ROI] or None."""
    nhood = np.asarray(nhood)[: pred.shape[0]]
    roi_shape = pred.shape[1:]
    neg = [min([0] + list(nhood[:, d])) for d in range(3)]
    pos = [max([0] + list(nhood[:, d])) for d in range(3)]
    chunk = [min(c, n) for c, n in zip(chunk, roi_shape)]
    factor = np.float32(1.0 / 255)
    floor, ceil = thresholds
    emap = np.zeros(roi_shape, np.uint8)
    emask = np.zeros(roi_shape, np.uint8)
    for org in scan_chunks(roi_shape, chunk):
        sl = tuple(slice(o, o + c) for o, c in zip(org, chunk))
        s = padded(seg, [r + o + n for r, o, n in zip(roi_begin, org, neg)], [c - n + p for c, n, p in zip(chunk, neg, pos)])
        affs = seg_to_affgraph(s, nhood).astype(np.float32)
        affs = affs[(slice(None),) + tuple(slice(-n, -n + c) for n, c in zip(neg, chunk))]
        p = pred[(slice(None),) + sl].astype(np.float32) * factor
        diff = np.sum((affs - p) ** 2, axis=0)
        if mask is not None:
            diff *= mask[sl]
        m = np.max(diff)
        if m > 0:
            diff /= m
        else:
            diff[:] = 0
        emask[sl] = ((diff > floor) & (diff < ceil)).astype(np.uint8)
        emap[sl] = (diff * 255 + 0).astype(np.uint8)
    return emap, emask


def compute_stats(array):
    """eval/compute_errors.py:226-239"""
    total_voxels = int(np.prod(array.shape))
    num_nonzero_voxels = array[array > 0].size
    return {"mean": float(np.mean(array)), "std": float(np.std(array)), "num_nonzero_voxels": num_nonzero_voxels,
            "total_voxels": total_voxels, "nonzero_ratio": num_nonzero_voxels / total_voxels}


def contingency(gt, seg, mask=None):
    """(gt id, seg id, count) of every pair, ascending, gt 0 left out; ids multiplied by the mask first (u64 wrap)"""
    g = np.asarray(gt, np.uint64).ravel()
    s = np.asarray(seg, np.uint64).ravel()
    if mask is not None:
        m = np.asarray(mask).ravel().astype(np.uint64)
        g, s = g * m, s * m
    keep = g != 0
    pairs, counts = np.unique(np.stack([g[keep], s[keep]], axis=1), axis=0, return_counts=True)
    return pairs[:, 0], pairs[:, 1], counts.astype(np.uint64)


def rand_voi(gt, seg, mask=None):
    """funlib.evaluate.rand_voi without voi_split_i / voi_merge_j: gt 0 ignored, seg 0 an ordinary label, VOI in bits"""
    gi, si, n = contingency(gt, seg, mask)
    p = n.astype(np.float64) / float(n.sum())
    _, ig = np.unique(gi, return_inverse=True)
    _, js = np.unique(si, return_inverse=True)
    a = np.bincount(ig, weights=p)
    b = np.bincount(js, weights=p)
    h_ab = -np.sum(p * np.log2(p))
    h_a = -np.sum(a * np.log2(a))
    h_b = -np.sum(b * np.log2(b))
    voi_split, voi_merge = h_ab - h_a, h_ab - h_b
    nvi_split = voi_split / h_ab if h_ab > 0 else 0.0
    nvi_merge = voi_merge / h_ab if h_ab > 0 else 0.0
    return {"rand_split": float(np.sum(p * p) / np.sum(a * a)), "rand_merge": float(np.sum(p * p) / np.sum(b * b)),
            "voi_split": float(voi_split), "voi_merge": float(voi_merge), "nvi_split": float(nvi_split),
            "nvi_merge": float(nvi_merge), "nvi_total": float(nvi_split + nvi_merge)}
