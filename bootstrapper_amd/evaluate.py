"""`bs evaluate`: scores of segmentations, against ground truth (Rand / VOI) or against the network's own output (error maps
against its affinities, or, opt-in, against its local shape descriptors), on the device.

Same command, flags, modes, config keys, dataset discovery, output datasets and JSON as the reference's bootstrapper/evaluate.py
(`get_seg_datasets` :16-21, `get_eval_config` :24-36, `run_gt_evaluation` :39-64, `run_pred_evaluation` :67-101,
`run_evaluation` :104-127, `evaluate` :130-159).  The volumes stream through one layer of chunks at a time:

  pred mode  the pred layer and the mask layer are read once and every segmentation is scored against them
             (csrc/eval.hip `bsmi_eval_aff_errors_u8`: diff, per-chunk maximum, both u8 outputs and the histograms that
             give the statistics exactly); the outputs are written behind the next layer's work.  A `3d_lsds` pred dataset
             takes the LSD form (`bsmi_eval_lsd_errors_u8`, gp/add_lsd_errors.py) when `[pred] lsd_errors = true` or
             `--lsd_errors` opts in: per chunk, over the chunk grown by `lsd_margin` (default (2, 50, 50) voxels, the
             reference's chunk + (4, 100, 100) request), the segmentation's own descriptors (sigma = `lsd_sigma` of
             [pred.params], else int(voxel_size[-1] * 10); downsample 2), the diff against pred, one maximum, the threshold,
             the in-plane opening and z closing, then the crop to the chunk.  The lsd package is restated (oracle/lsd_ref.py,
             tests/lsd_errors_ref.py), not pinned: that is why the form is opt-in
  gt mode    (gt, seg) pair counts per tile on the device (`bsmi_eval_pairs_u64`), merged on the host in exact integers;
             Rand / VOI from the merged table in float64, in ascending (gt, seg) order

Not part of this engine, refused before any work: `3d_lsds` pred datasets without the opt-in, and `gt.skeletons_file` (ERL).
One deliberate difference: an `out_result` that would overwrite the config file (a config name without `.toml`) is refused.
"""
import concurrent.futures as cf
import ctypes as C
import glob
import json
import math
import os
from pprint import pprint

import click
import numpy as np

from .segment import load_toml
from .zarr_io import open_ds, prepare_ds

DEFAULT_NEIGHBORHOOD = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0], [0, 8, 0], [0, 0, 8]]
DEFAULT_THRESHOLDS = [0.1, 1.0]
PAIR_CAPACITY = 1 << 22      # slots of the device pair table (3 x 32 MiB + the read-out buffers)
GT_TILE_VOXELS = 1 << 24     # voxels of one gt-mode tile before any halving on overflow
LSD_SCRATCH_BYTES = 1 << 30  # device scratch of the LSD form: a layer's chunks go through in groups that stay below this
WRITES_IN_FLIGHT = 8         # output pieces queued behind the device
LSD_DOWNSAMPLE = 2           # eval/compute_errors.py:159
LSD_MARGIN = [2, 50, 50]     # (input_shape - output_shape) / 2 of eval/compute_errors.py:89-90, voxels
LSD_BLOCK_CELLS = (2, 8, 16)  # lsd_desc_kernel: cells of one block; its window and weight tables share LSD_LDS_BYTES
LSD_LDS_BYTES = 72704
LSD_REFUSAL = "3d_lsds error maps are not part of this engine (affinities only)"


def get_seg_datasets(seg_datasets_prefix):
    seg_datasets = []
    for ds in sorted(glob.glob(f"{seg_datasets_prefix}*/*/.zarray")):
        if "__vs__" not in ds:  # skip pred errors
            seg_datasets.append(os.path.dirname(ds))
    return seg_datasets


def get_eval_config(config_file, mode, **kwargs):
    config = load_toml(config_file)
    for key, value in kwargs.items():
        if value is not None:
            config[key] = value
    if "out_result" not in config:
        config["out_result"] = config_file.replace("04_eval_", f"results_{mode}_").replace(".toml", ".json")
    return config


def _check_scope(config, mode):
    """out-of-scope inputs, refused before any dataset is read or written"""
    if mode == "gt":
        gt = config.get("gt") or {}
        if gt.get("skeletons_file") is not None:
            raise NotImplementedError(f"gt.skeletons_file ({gt['skeletons_file']}): skeleton (ERL) evaluation is not part of this engine")
        if gt.get("labels_dataset") is None:
            raise AssertionError("Either labels_dataset or skeletons_file must be provided")
    else:
        pred_dataset = config["pred"]["pred_dataset"]
        name = os.path.basename(pred_dataset.rstrip("/"))
        if "3d_lsds" in name:
            if not config["pred"].get("lsd_errors"):
                raise NotImplementedError(f"{pred_dataset}: {LSD_REFUSAL}; opt in with [pred] lsd_errors = true or --lsd_errors")
        elif "3d_affs" not in name:
            raise ValueError(f"Unknown type for {pred_dataset}")


# ---- ROIs (world units, (offset, shape)) ---------------------------------------------------------------------------------

def _intersect(a, b):
    lo = [max(x, y) for x, y in zip(a[0], b[0])]
    hi = [min(x + s, y + t) for x, s, y, t in zip(a[0], a[1], b[0], b[1])]
    return lo, [max(0, h - l) for l, h in zip(lo, hi)]


def _voxel_begin(ds, roi):
    return [(o - off) // v for o, off, v in zip(roi[0], ds.offset, ds.voxel_size)]


def _same_voxel_size(named):
    sizes = {n: tuple(ds.voxel_size) for n, ds in named if ds is not None}
    if len(set(sizes.values())) > 1:
        raise ValueError(f"voxel sizes differ: {sizes}")


def _read_padded(ds, begin, shape, dtype):
    """ds[..., begin : begin + shape] (spatial; every channel) as `dtype`, zeros beyond the dataset (gp.Pad)"""
    lead = (slice(None),) * (len(ds.shape) - 3)
    out = np.zeros(list(ds.shape[:-3]) + list(shape), dtype=dtype)
    lo = [max(0, b) for b in begin]
    hi = [min(n, b + s) for n, b, s in zip(ds.shape[-3:], begin, shape)]
    if any(h <= l for l, h in zip(lo, hi)):
        return out
    key = lead + tuple(slice(l, h) for l, h in zip(lo, hi))
    dst = lead + tuple(slice(l - b, h - b) for l, h, b in zip(lo, hi, begin))
    if ds.dtype == dtype:
        ds.read_into(key, out[dst])
    else:
        out[dst] = ds[key].astype(dtype)
    return out


def _as_mask_u8(a, name):
    if a.dtype == np.uint8:
        return a
    if a.dtype.kind not in "biu" or (a.size and int(a.max()) > 255) or (a.size and a.dtype.kind == "i" and int(a.min()) < 0):
        raise ValueError(f"mask {name}: values must be integers in [0, 255] (dtype {a.dtype})")
    return a.astype(np.uint8)


# ---- device -----------------------------------------------------------------------------------------------------------

class EvalDevice:
    """a bsmi_eval handle with torch for the buffers and the stream"""

    def __init__(self, device=0, pair_capacity=PAIR_CAPACITY):
        import torch
        from . import _lib
        self.torch, self.lib = torch, _lib
        self.dev = torch.device("cuda", device)
        self.cap = int(pair_capacity)
        h = C.c_void_p()
        _lib.check(_lib.lib.bsmi_eval_create(device, self.cap, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.lib.lib.bsmi_eval_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    @property
    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def to_dev(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a))
        return t.to(self.dev, non_blocking=False)

    def aff_errors(self, seg_t, seg_origin, pred_t, mask_t, offsets, chunk, thresholds, count_z_end, emap_t, emask_t, hist_t):
        L = self.lib
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        offs = (C.c_int32 * (3 * len(offsets)))(*[int(v) for o in offsets for v in o])
        L.check(L.lib.bsmi_eval_aff_errors_u8(
            self.h, ptr(seg_t), L.i64x3(seg_t.shape), L.i64x3(seg_origin), ptr(pred_t), int(pred_t.shape[0]),
            L.i64x3(pred_t.shape[1:]), ptr(mask_t), offs, L.i64x3(chunk),
            float(thresholds[0]), float(thresholds[1]), int(count_z_end), ptr(emap_t), ptr(emask_t), ptr(hist_t), self.stream))

    def lsd_errors(self, seg_t, seg_origin, pred_t, mask_t, tile, chunk, lsd, thresholds, count_z_end, emap_t, emask_t, hist_t,
                   debug=None, scratch_bytes=LSD_SCRATCH_BYTES):
        """lsd: lsd_setup()'s dict.  debug: lsd_debug_buffers() or None"""
        L = self.lib
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])  # noqa: E731
        dbg = debug or {}
        L.check(L.lib.bsmi_eval_lsd_errors_u8(
            self.h, ptr(seg_t), L.i64x3(seg_t.shape), L.i64x3(seg_origin), ptr(pred_t), ptr(mask_t), L.i64x3(tile), L.i64x3(chunk),
            L.i64x3(lsd["margin"]), L.i64x3(lsd["context"]), f3(lsd["sigma"]), f3(lsd["voxel_size"]), int(lsd["downsample"]),
            float(thresholds[0]), float(thresholds[1]), int(count_z_end), int(scratch_bytes), ptr(emap_t), ptr(emask_t), ptr(hist_t),
            ptr(dbg.get("desc")), ptr(dbg.get("diff")), ptr(dbg.get("max")), ptr(dbg.get("raw")), self.stream))

    def lsd_debug_buffers(self, tile, chunk, margin):
        """the per-stage outputs of lsd_errors, per chunk over its grown region, chunks in the order (jz * ncy + jy) * ncx + jx"""
        torch = self.torch
        c = [min(a, b) for a, b in zip(chunk, tile)]
        n = int(np.prod([-(-t // k) for t, k in zip(tile, c)]))
        g = [k + 2 * m for k, m in zip(c, margin)]
        return {"desc": torch.zeros([n, 10] + g, dtype=torch.float32, device=self.dev),
                "diff": torch.zeros([n] + g, dtype=torch.float32, device=self.dev),
                "max": torch.zeros([n], dtype=torch.float32, device=self.dev),
                "raw": torch.zeros([n] + g, dtype=torch.uint8, device=self.dev)}

    def pairs(self, gt_t, seg_t, mask_t):
        """-> (gt ids, seg ids, counts) of one tile (u64 numpy, unordered); raises BsmiError(ERR_OVERFLOW) if the table is full"""
        L, torch = self.lib, self.torch
        st = self.stream
        L.check(L.lib.bsmi_eval_pairs_u64(self.h, C.c_void_p(gt_t.data_ptr()), C.c_void_p(seg_t.data_ptr()),
                                          C.c_void_p(mask_t.data_ptr()) if mask_t is not None else None, L.i64x3(gt_t.shape), 1, st))
        out = torch.empty((3, self.cap), dtype=torch.int64, device=self.dev)
        n = torch.zeros(1, dtype=torch.int64, device=self.dev)
        L.check(L.lib.bsmi_eval_pairs_read(self.h, C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()),
                                           C.c_void_p(out[2].data_ptr()), self.cap, C.c_void_p(n.data_ptr()), st))
        L.check(L.lib.bsmi_eval_status(self.h, st))
        k = int(n.item())
        host = out[:, :k].cpu().numpy().view(np.uint64)
        return host[0], host[1], host[2]


# ---- statistics and metrics ---------------------------------------------------------------------------------------------

def stats_from_histogram(hist):
    """compute_stats (eval/compute_errors.py:226-239) of a u8 dataset from its value histogram: the mean exactly (an integer
    sum over the count), the standard deviation about that mean"""
    h = [int(v) for v in hist]
    total = sum(h)
    s = sum(i * c for i, c in enumerate(h))
    mean = s / total
    var = math.fsum(c * (i - mean) ** 2 for i, c in enumerate(h) if c) / total
    nonzero = total - h[0]
    return {"mean": float(mean), "std": float(math.sqrt(var)), "num_nonzero_voxels": nonzero, "total_voxels": total,
            "nonzero_ratio": nonzero / total}


def merge_pairs(parts):
    """concatenated (gt, seg, count) triples -> the same pairs once each, ascending (gt, seg), counts summed exactly"""
    if not parts:
        z = np.zeros(0, np.uint64)
        return z, z, z
    g = np.concatenate([p[0] for p in parts])
    s = np.concatenate([p[1] for p in parts])
    n = np.concatenate([p[2] for p in parts])
    if g.size == 0:
        return g, s, n
    order = np.lexsort((s, g))
    g, s, n = g[order], s[order], n[order]
    start = np.flatnonzero(np.concatenate([[True], (g[1:] != g[:-1]) | (s[1:] != s[:-1])]))
    return g[start], s[start], np.add.reduceat(n, start).astype(np.uint64)


def rand_voi_from_table(g, s, n):
    """funlib.evaluate.rand_voi from the pair table (gt 0 already left out), float64 in ascending (gt, seg) order:
    rand_split = sum n_ij^2 / sum a_i^2, rand_merge = sum n_ij^2 / sum b_j^2, voi_split = H(seg|gt), voi_merge = H(gt|seg) in
    bits, nvi_* = each VOI term / H(gt, seg) (0 when that is 0), nvi_total = their sum"""
    if n.size == 0:
        nan = float("nan")
        return {"rand_split": nan, "rand_merge": nan, "voi_split": 0.0, "voi_merge": 0.0, "nvi_split": 0.0, "nvi_merge": 0.0,
                "nvi_total": 0.0}
    p = n.astype(np.float64) / float(int(n.sum(dtype=np.uint64)))
    _, ig = np.unique(g, return_inverse=True)
    _, js = np.unique(s, return_inverse=True)
    a = np.bincount(ig, weights=p)
    b = np.bincount(js, weights=p)
    h_ab = float(-np.sum(p * np.log2(p)))
    h_a = float(-np.sum(a * np.log2(a)))
    h_b = float(-np.sum(b * np.log2(b)))
    sum_p2 = float(np.sum(p * p))
    voi_split, voi_merge = h_ab - h_a, h_ab - h_b
    nvi_split = voi_split / h_ab if h_ab > 0 else 0.0
    nvi_merge = voi_merge / h_ab if h_ab > 0 else 0.0
    return {"rand_split": sum_p2 / float(np.sum(a * a)), "rand_merge": sum_p2 / float(np.sum(b * b)), "voi_split": voi_split,
            "voi_merge": voi_merge, "nvi_split": nvi_split, "nvi_merge": nvi_merge, "nvi_total": nvi_split + nvi_merge}


# ---- gt mode ----------------------------------------------------------------------------------------------------------

def compute_metrics(seg_dataset, gt_labels_dataset, mask_dataset=None, device=0, engine=None, tile_voxels=GT_TILE_VOXELS):
    """eval/compute_metrics.py:73-122 for labels: {"voi": rand_voi report} over seg.roi & gt.roi & mask.roi"""
    seg_ds, gt_ds = open_ds(seg_dataset), open_ds(gt_labels_dataset)
    mask_ds = None if mask_dataset is None else open_ds(mask_dataset)
    _same_voxel_size([(seg_dataset, seg_ds), (gt_labels_dataset, gt_ds), (mask_dataset, mask_ds)])
    roi = _intersect(seg_ds.roi, gt_ds.roi)
    if mask_ds is not None:
        roi = _intersect(roi, mask_ds.roi)
    vs = seg_ds.voxel_size
    shape = [s // v for s, v in zip(roi[1], vs)]
    eng = engine or EvalDevice(device)
    parts = []
    sb, gb = _voxel_begin(seg_ds, roi), _voxel_begin(gt_ds, roi)
    mb = None if mask_ds is None else _voxel_begin(mask_ds, roi)
    plane = max(1, shape[1] * shape[2])
    z = 0
    depth = max(1, tile_voxels // plane)
    while z < shape[0] and all(shape):
        d = min(depth, shape[0] - z)
        tile = [d, shape[1], shape[2]]
        gt = _read_padded(gt_ds, [gb[0] + z, gb[1], gb[2]], tile, np.uint64)
        seg = _read_padded(seg_ds, [sb[0] + z, sb[1], sb[2]], tile, np.uint64)
        mask = None if mask_ds is None else _as_mask_u8(_read_padded(mask_ds, [mb[0] + z, mb[1], mb[2]], tile, mask_ds.dtype), mask_dataset)
        try:
            parts.append(eng.pairs(eng.to_dev(gt), eng.to_dev(seg), None if mask is None else eng.to_dev(mask)))
        except eng.lib.BsmiError as e:
            if e.code != eng.lib.ERR_OVERFLOW or d == 1:
                raise
            depth = max(1, d // 2)   # more distinct pairs than the table holds: the same slices in thinner tiles
            continue
        z += d
    return {"voi": rand_voi_from_table(*merge_pairs(parts))}


def run_gt_evaluation(config, seg_ds, device=0, engine=None):
    gt_labels_dataset = config["gt"].get("labels_dataset")
    gt_skeletons_file = config["gt"].get("skeletons_file")
    mask_dataset = config.get("mask_dataset")
    if gt_skeletons_file is not None:
        raise NotImplementedError(f"gt.skeletons_file ({gt_skeletons_file}): skeleton (ERL) evaluation is not part of this engine")
    if gt_labels_dataset is None:
        raise AssertionError("Either labels_dataset or skeletons_file must be provided")
    metrics = compute_metrics(seg_ds, gt_labels_dataset, mask_dataset, device=device, engine=engine)
    return {"seg_ds": seg_ds, "labels_ds": gt_labels_dataset, "skeletons_file": gt_skeletons_file, "mask_ds": mask_dataset,
            "metrics": metrics}


# ---- pred mode --------------------------------------------------------------------------------------------------------

def scan_origins(n, c):
    """gp.Scan along one axis of extent n with chunk c (clamped to n): 0, c, 2c, ... and the last chunk moved back to end at n"""
    c = min(c, n)
    return list(range(0, n - c, c)) + [n - c]


class _Writes:
    """write-behind of host arrays through ZarrArray.write_from, at most WRITES_IN_FLIGHT pieces queued"""

    def __init__(self):
        self.pool = cf.ThreadPoolExecutor(max_workers=4, thread_name_prefix="bsmi-eval-write")
        self.futures = []

    def submit(self, ds, key, array):
        while len(self.futures) >= WRITES_IN_FLIGHT:
            self.futures.pop(0).result()
        self.futures.append(self.pool.submit(ds.write_from, key, array))

    def drain(self):
        while self.futures:
            self.futures.pop(0).result()

    def close(self):
        try:
            self.drain()
        finally:
            self.pool.shutdown(wait=True)


def lsd_setup(voxel_size, lsd_sigma=None, lsd_margin=None, downsample=LSD_DOWNSAMPLE):
    """the LSD form's parameters as eval/compute_errors.py:60 and AddLSDErrors.setup / prepare derive them: one sigma for the
    three axes, the context 3 sigma in world units snapped to voxels by shrinking"""
    sigma = lsd_sigma if lsd_sigma is not None else int(voxel_size[-1] * 10)
    if isinstance(sigma, (list, tuple)) or not sigma > 0:
        raise ValueError(f"lsd_sigma must be one positive number (got {sigma!r})")
    margin = [int(m) for m in (lsd_margin if lsd_margin is not None else LSD_MARGIN)]
    if len(margin) != 3 or min(margin) < 0:
        raise ValueError(f"lsd_margin must be three non-negative voxel counts (got {lsd_margin!r})")
    return {"sigma": [sigma] * 3, "voxel_size": [int(v) for v in voxel_size], "downsample": int(downsample), "margin": margin,
            "context": [int(math.floor(3 * sigma / v)) for v in voxel_size]}


def lsd_check_geometry(lsd, chunk, what):
    """what the lsd package asserts and what lsd_desc_kernel can hold, as a ValueError before anything is written"""
    df = lsd["downsample"]
    for d, ax in enumerate("zyx"):
        grown = chunk[d] + 2 * lsd["margin"][d]
        if grown % df:
            raise ValueError(f"{what}: chunk + 2 * lsd_margin = {grown} voxels along {ax} is not a multiple of the downsample factor {df}")
        if lsd["context"][d] % df:
            raise ValueError(f"{what}: the context floor(3 * sigma / voxel_size) = {lsd['context'][d]} voxels along {ax} is not a multiple of "
                             f"the downsample factor {df}")
    r = [int(3.0 * (s / (v * df)) + 0.5) for s, v in zip(lsd["sigma"], lsd["voxel_size"])]
    # weight tables (z, y: 3 per tap; x: 3 x 64 partial sums per group of 6 taps) in float64, then the window and its pad
    need = 8 * (3 * (2 * r[0] + 1 + 2 * r[1] + 1) + 192 * -(-(2 * r[2] + 1) // 6)) + 4 * (int(np.prod([b + 2 * x for b, x in zip(LSD_BLOCK_CELLS, r)])) + 8)
    if need > LSD_LDS_BYTES or max(r) > 512:
        raise ValueError(f"{what}: the LSD window radius {r} (sub-grid cells) is above the kernel's limit: its window needs {need} bytes "
                         f"of LDS, {LSD_LDS_BYTES} are there")


def compute_errors(seg_datasets, pred_dataset, mask_dataset, out_datasets, thresholds=(0.1, 1.0), roi_offset=None, roi_shape=None,
                   aff_neighborhood=None, device=0, engine=None, whole_roi=False, lsd_errors=False, lsd_sigma=None, lsd_margin=None,
                   **kwargs):
    """eval/compute_errors.py:25-223 for several segmentations at once: out_datasets[i] = (error_map, error_mask) dataset
    paths of seg_datasets[i].  -> [(error_map stats, error_mask stats)] per segmentation.  The dataset's name chooses the form:
    `3d_affs` the affinity form, `3d_lsds` the LSD form (only with lsd_errors = True).
    One layer of chunks is on the device at a time; whole_roi = True hands the whole ROI over as one tile (same outputs)."""
    pred_ds = open_ds(pred_dataset)
    name = os.path.basename(pred_dataset.rstrip("/"))
    is_lsd = "3d_lsds" in name
    if is_lsd and not lsd_errors:
        raise NotImplementedError(f"{pred_dataset}: {LSD_REFUSAL}; opt in with [pred] lsd_errors = true or --lsd_errors")
    if not is_lsd and "3d_affs" not in name:
        raise ValueError(f"Unknown type for {pred_dataset}")
    if pred_ds.dtype != np.uint8:
        raise ValueError(f"{pred_dataset}: pred datasets must be uint8 (got {pred_ds.dtype})")
    if len(pred_ds.shape) != 4:
        raise ValueError(f"{pred_dataset}: expected [channels][z][y][x], got shape {pred_ds.shape}")
    K = pred_ds.shape[0]
    nhood = lsd = None
    if is_lsd:
        if K != 10:
            raise ValueError(f"{pred_dataset}: an LSD pred dataset has 10 channels (got {K})")
        lsd = lsd_setup(pred_ds.voxel_size, lsd_sigma, lsd_margin)
    else:
        nhood = [list(map(int, o)) for o in (aff_neighborhood if aff_neighborhood is not None else DEFAULT_NEIGHBORHOOD)]
        if len(nhood) < K:
            raise ValueError(f"aff_neighborhood has {len(nhood)} offsets, {pred_dataset} has {K} channels")
        nhood = nhood[:K]
        if K > 16:
            raise ValueError(f"{pred_dataset}: at most 16 affinity channels")
    seg_dss = [open_ds(s) for s in seg_datasets]
    mask_ds = None if mask_dataset is None else open_ds(mask_dataset)
    _same_voxel_size([(pred_dataset, pred_ds), (mask_dataset, mask_ds)] + list(zip(seg_datasets, seg_dss)))
    vs = pred_ds.voxel_size
    mask_roi = pred_ds.roi if mask_ds is None else mask_ds.roi
    rois = []
    for sd in seg_dss:
        roi = _intersect(_intersect(pred_ds.roi, sd.roi), mask_roi)
        if roi_offset is not None:
            roi = _intersect((list(roi_offset), list(roi_shape)), roi)
        rois.append(roi)
    if lsd is not None:
        for sd_name, roi in zip(seg_datasets, rois):
            shape = [s // v for s, v in zip(roi[1], vs)]
            lsd_check_geometry(lsd, [min(c, n) for c, n in zip(pred_ds.chunks[1:], shape)], f"{sd_name} against {pred_dataset}")
    shape_groups = {}
    for i, roi in enumerate(rois):   # segmentations over the same ROI share the pred / mask reads
        shape_groups.setdefault((tuple(roi[0]), tuple(roi[1])), []).append(i)
    results = [None] * len(seg_dss)
    eng = engine or EvalDevice(device)
    for (off, size), members in shape_groups.items():
        roi = (list(off), list(size))
        for i, st in zip(members, _errors_over_roi(eng, pred_ds, mask_ds, mask_dataset, [seg_dss[i] for i in members],
                                                   [out_datasets[i] for i in members], roi, nhood, thresholds, whole_roi, lsd)):
            results[i] = st
    return results


def _errors_over_roi(eng, pred_ds, mask_ds, mask_name, seg_dss, outs, roi, nhood, thresholds, whole_roi=False, lsd=None):
    """lsd = None: the affinity form with the neighbourhood nhood; else the LSD form with lsd_setup()'s parameters"""
    torch = eng.torch
    vs = pred_ds.voxel_size
    shape = [s // v for s, v in zip(roi[1], vs)]
    if min(shape) <= 0:
        raise ValueError(f"the ROI {roi} is empty")
    if shape[1] > (1 << 20) or shape[2] > (1 << 20):
        raise ValueError(f"ROI {shape} voxels: rows and sections beyond 2^20 voxels are not supported")
    chunk = [min(c, n) for c, n in zip(pred_ds.chunks[1:], shape)]
    if lsd is None:
        grow = [0, 0, 0]   # pred and mask cover the tile itself
        neg = [min([0] + [o[d] for o in nhood]) for d in range(3)]
        pos = [max([0] + [o[d] for o in nhood]) for d in range(3)]
    else:
        grow = lsd["margin"]   # they cover every chunk's grown region, the segmentation its label array
        pos = [m + c for m, c in zip(lsd["margin"], lsd["context"])]
        neg = [-p for p in pos]
    outs_ds = []
    for sd, (map_path, mask_path) in zip(seg_dss, outs):
        keep = dict(shape=shape, offset=roi[0], voxel_size=vs, axis_names=sd.axis_names[-3:], units=sd.units[-3:],
                    chunk_shape=chunk, dtype=np.uint8)
        outs_ds.append((prepare_ds(map_path, **keep), prepare_ds(mask_path, **keep)))
    pb = _voxel_begin(pred_ds, roi)
    mb = None if mask_ds is None else _voxel_begin(mask_ds, roi)
    sbs = [_voxel_begin(sd, roi) for sd in seg_dss]
    hists = [torch.zeros(257, dtype=torch.int64, device=eng.dev) for _ in seg_dss]
    zs = [0] if whole_roi else scan_origins(shape[0], chunk[0])
    writes = _Writes()
    try:
        for li, z in enumerate(zs):
            tz = shape[0] if whole_roi else chunk[0]
            keep_z = zs[li + 1] - z if li + 1 < len(zs) else tz   # the next layer rewrites the slices after these
            if li + 1 == len(zs) and len(zs) > 1:
                writes.drain()   # the snapped last layer shares a chunk with the one before: no two writers on one chunk
            tile = [tz, shape[1], shape[2]]
            grown = [t + 2 * g for t, g in zip(tile, grow)]
            if lsd is None:
                pred = np.empty([pred_ds.shape[0]] + tile, np.uint8)
                pred_ds.read_into((slice(None), slice(pb[0] + z, pb[0] + z + tz), slice(pb[1], pb[1] + shape[1]),
                                   slice(pb[2], pb[2] + shape[2])), pred)
            else:   # real values inside the dataset, also outside the ROI; zeros beyond it (gp.Pad(pred, None))
                pred = _read_padded(pred_ds, [pb[0] + z - grow[0], pb[1] - grow[1], pb[2] - grow[2]], grown, np.uint8)
            pred_t = eng.to_dev(pred)
            mask_t = None
            if mask_ds is not None:
                mask_t = eng.to_dev(_as_mask_u8(_read_padded(mask_ds, [mb[0] + z - grow[0], mb[1] - grow[1], mb[2] - grow[2]], grown,
                                                             mask_ds.dtype), mask_name))
            for sd, sb, hist, (map_ds, msk_ds) in zip(seg_dss, sbs, hists, outs_ds):
                seg_shape = [t - n + p for t, n, p in zip(tile, neg, pos)]
                seg = _read_padded(sd, [sb[0] + z + neg[0], sb[1] + neg[1], sb[2] + neg[2]], seg_shape, np.uint64)
                seg_t = eng.to_dev(seg)
                emap_t = torch.empty(tile, dtype=torch.uint8, device=eng.dev)
                emask_t = torch.empty(tile, dtype=torch.uint8, device=eng.dev)
                if lsd is None:
                    eng.aff_errors(seg_t, neg, pred_t, mask_t, nhood, chunk, thresholds, keep_z, emap_t, emask_t, hist)
                else:
                    eng.lsd_errors(seg_t, neg, pred_t, mask_t, tile, chunk, lsd, thresholds, keep_z, emap_t, emask_t, hist)
                key = (slice(z, z + keep_z), slice(0, shape[1]), slice(0, shape[2]))
                writes.submit(map_ds, key, emap_t[:keep_z].cpu().numpy())
                writes.submit(msk_ds, key, emask_t[:keep_z].cpu().numpy())
        writes.drain()
        if lsd is not None:
            eng.lib.check(eng.lib.lib.bsmi_eval_status(eng.h, eng.stream))   # more distinct labels than the id table holds
    finally:
        writes.close()
    out = []
    for hist in hists:
        h = hist.cpu().numpy()
        total = int(np.prod(shape))
        assert int(h[:256].sum()) == total, (int(h[:256].sum()), total)
        ones = int(h[256])
        out.append((stats_from_histogram(h[:256]), stats_from_histogram([total - ones, ones])))
    return out


def _pred_outputs(seg_ds, pred_dataset):
    pred_name = os.path.basename(pred_dataset)
    return (os.path.join(seg_ds + f"__vs__{pred_name}", "error_map"), os.path.join(seg_ds + f"__vs__{pred_name}", "error_mask"))


def run_pred_evaluations(config, seg_datasets, device=0, engine=None):
    """run_pred_evaluation (evaluate.py:67-101) for every segmentation, the pred and mask layers read once for all of them"""
    pred_dataset = config["pred"]["pred_dataset"]
    thresholds = config["pred"].get("thresholds", DEFAULT_THRESHOLDS)
    params = config["pred"].get("params", {})
    mask_dataset = config.get("mask_dataset")
    outs = [_pred_outputs(s, pred_dataset) for s in seg_datasets]
    stats = compute_errors(seg_datasets, pred_dataset, mask_dataset, outs, thresholds=thresholds, device=device, engine=engine,
                           lsd_errors=bool(config["pred"].get("lsd_errors", False)), **params)
    entries = []
    for seg_ds, (map_ds, mask_ds), (map_stats, mask_stats) in zip(seg_datasets, outs, stats):
        # the reference's dict literal names "mask_ds" twice: the key keeps its first place and takes the error-mask path
        entries.append({"seg_ds": seg_ds, "pred_ds": pred_dataset, "mask_ds": mask_ds, "map_ds": map_ds, "thresholds": thresholds,
                        "error_map": map_stats, "error_mask": mask_stats})
    return entries


def run_pred_evaluation(config, seg_ds, device=0, engine=None):
    return run_pred_evaluations(config, [seg_ds], device, engine)[0]


def run_evaluation(config_file, mode="pred", device=0, **kwargs):
    lsd_errors = kwargs.pop("lsd_errors", None)
    config = get_eval_config(config_file, mode, **kwargs)
    if lsd_errors and mode == "pred":
        config.setdefault("pred", {})["lsd_errors"] = True
    out_result = kwargs.get("out_result") or config["out_result"]
    if os.path.abspath(out_result) == os.path.abspath(config_file):
        raise ValueError(f"out_result {out_result} would overwrite the config file: name the config 04_eval_*.toml or pass --out_result")
    _check_scope(config, mode)
    if "seg_datasets" in config:
        seg_datasets = [ds.rstrip("/") for ds in config["seg_datasets"]]
    else:
        seg_datasets = get_seg_datasets(config["seg_datasets_prefix"])
    eng = EvalDevice(device)
    try:
        for seg_ds in seg_datasets:
            print(f"Evaluating {seg_ds}")
        if mode == "pred":
            entries = run_pred_evaluations(config, seg_datasets, device, eng) if seg_datasets else []
        elif mode == "gt":
            entries = [run_gt_evaluation(config, s, device, eng) for s in seg_datasets]
        else:
            raise ValueError(f"unknown mode {mode!r}")
    finally:
        eng.close()
    seg_stats = {}
    for seg_ds, stats in zip(seg_datasets, entries):
        print(f"Stats for {seg_ds}:")
        pprint(stats)
        seg_stats[seg_ds] = stats
    print(f"Saving stats to {out_result}")
    with open(out_result, "w") as f:
        json.dump(seg_stats, f, indent=4)
    return out_result


def eval_modes(config_file, gt=False, pred=False):
    """evaluate.py:142-156: the flags choose; else the config sections present, gt before pred; else pred"""
    if gt or pred:
        return [m for m, on in (("gt", gt), ("pred", pred)) if on]
    config = load_toml(config_file)
    present = [m for m in ("gt", "pred") if config.get(m)]
    return present or ["pred"]


@click.command()
@click.argument("config_file", type=click.Path(exists=True, file_okay=True, dir_okay=False))
@click.option("--gt", "-gt", is_flag=True, help="Evaluate only against ground-truth")
@click.option("--pred", "-p", is_flag=True, help="Evaluate only against predictions")
@click.option("--out_result", "-o", type=click.Path())
@click.option("--lsd_errors", is_flag=True, help="Score against a 3d_lsds pred dataset (LSD error maps; same as [pred] lsd_errors = true)")
def evaluate(config_file, gt, pred, out_result=None, lsd_errors=False):
    """Evaluate segmentations as specified in the config file."""
    for mode in eval_modes(config_file, gt, pred):
        run_evaluation(config_file, mode, out_result=out_result, lsd_errors=lsd_errors or None)
