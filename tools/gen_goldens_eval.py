#!/usr/bin/env python3
"""One-command pin for `bs evaluate`: run this WHERE gunpowder, funlib.evaluate, funlib.persistence AND the reference package
`bootstrapper` ARE INSTALLED and commit the file it writes, tests/golden/eval_cases.npz.  From then on tests/test_eval_pin.py
holds tests/eval_ref.py -- and through it the HIP kernels of csrc/eval.hip, which tests/test_evaluate_gpu.py holds bit-equal to
it -- to the reference's own `compute_errors(..., return_arrays=True)` and `funlib.evaluate.rand_voi`; until then that test
reports "parity UNPINNED".

    python tools/gen_goldens_eval.py            # -> tests/golden/eval_cases.npz, or a clear "not installed" message

What the cases decide (the restated choices of tests/eval_ref.py):
  * gp.Scan's chunk placement on ROIs that are not a multiple of the chunk (the last chunk moved back, the later chunk wins);
  * the region the normalising maximum is taken over;
  * gp.Normalize's factor and the f32 order of AddAffErrors._create_diff, with both offset signs and with a mask;
  * the rand_voi / nvi formulas (gt 0 ignored, seg 0 an ordinary label).
Inputs are made by numpy alone (seeded); the arrays stored are inputs and the reference's outputs -- data, not source.
"""
import json
import os
import sys
import tempfile

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "eval_cases.npz")
POS = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0], [0, 8, 0], [0, 0, 8]]
NEG = [[-o for o in off] for off in POS]
VOXEL_SIZE = (4, 2, 2)
# (seed, seg shape, ROI begin inside seg, ROI shape, chunk, neighbourhood, masked, thresholds)
ERROR_CASES = [
    (1, (29, 64, 80), (3, 7, 9), (23, 50, 61), (10, 32, 32), POS, False, (0.1, 1.0)),
    (2, (29, 64, 80), (3, 7, 9), (23, 50, 61), (10, 32, 32), NEG, True, (0.1, 1.0)),
    (3, (23, 50, 61), (0, 0, 0), (23, 50, 61), (10, 32, 32), NEG, False, (0.05, 0.9)),
    (4, (20, 40, 40), (0, 0, 0), (20, 40, 40), (8, 24, 24), POS, True, (0.2, 0.8)),
]
VOI_CASES = [(5, (12, 40, 50), 20, 35), (6, (6, 30, 30), 5, 60)]


def blobs(rng, shape, n):
    """Voronoi-like ids (anisotropic distance), some voxels 0"""
    pts = np.stack([rng.integers(0, s, n) for s in shape], 1)
    ids = rng.integers(1, 10 * n + 1, n).astype(np.uint64)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3)
    d = ((grid[:, None, :] - pts[None, :, :]) ** 2 * np.array([16, 1, 1])).sum(-1)
    out = ids[np.argmin(d, 1)].reshape(shape)
    out[rng.random(shape) < 0.02] = 0
    return out


def make_error_case(seed, seg_shape, roi_begin, roi_shape, masked):
    rng = np.random.default_rng(seed)
    seg = blobs(rng, seg_shape, 40)
    pred = rng.integers(0, 256, (6,) + tuple(roi_shape), dtype=np.uint8)
    mask = rng.integers(0, 2, roi_shape).astype(np.uint8) if masked else None
    return seg, pred, mask


def make_voi_case(seed, shape, n_gt, n_seg):
    rng = np.random.default_rng(seed)
    gt, seg = blobs(rng, shape, n_gt), blobs(rng, shape, n_seg)
    seg[: shape[0] // 3] = 0               # seg 0 is an ordinary label
    return gt, seg


def main():
    missing = []
    for name in ("gunpowder", "funlib.evaluate", "funlib.persistence", "bootstrapper.eval.compute_errors"):
        try:
            __import__(name)
        except ImportError as exc:
            missing.append(f"{name} ({exc})")
    if missing:
        print("not installed here: " + "; ".join(missing) + ".  Nothing written.  Run this script where the reference's "
              "evaluation stack is installed and commit tests/golden/eval_cases.npz.")
        return 2
    from funlib.evaluate import rand_voi
    from funlib.persistence import prepare_ds
    from funlib.geometry import Coordinate
    from bootstrapper.eval.compute_errors import compute_errors

    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, (seed, seg_shape, roi_begin, roi_shape, chunk, nhood, masked, thresholds) in enumerate(ERROR_CASES):
            seg, pred, mask = make_error_case(seed, seg_shape, roi_begin, roi_shape, masked)
            store = os.path.join(tmp, f"case{i}.zarr")
            vs = Coordinate(VOXEL_SIZE)
            roi_off = Coordinate(roi_begin) * vs

            def write(name, a, offset, chunks):
                ds = prepare_ds(os.path.join(store, name), shape=a.shape[-3:] if a.ndim == 3 else a.shape, offset=offset,
                                voxel_size=vs, dtype=a.dtype, chunk_shape=chunks)
                ds[ds.roi] = a
                return os.path.join(store, name)

            seg_path = write("seg", seg, Coordinate((0, 0, 0)), (8, 16, 16))
            pred_path = write("pred/3d_affs", pred, roi_off, (6,) + tuple(chunk))
            mask_path = write("mask", mask, roi_off, tuple(roi_shape)) if masked else None
            batch = compute_errors(seg_path, pred_path, mask_path, os.path.join(store, "out/error_map"),
                                   os.path.join(store, "out/error_mask"), thresholds=thresholds, return_arrays=True,
                                   aff_neighborhood=nhood)
            maps = [a for k, a in batch.arrays.items() if "MAP" in str(k)]
            masks = [a for k, a in batch.arrays.items() if "MASK" in str(k) and "LABELS" not in str(k)]
            key = f"errors{i}"
            out[key + "/seg"], out[key + "/pred"] = seg, pred
            if masked:
                out[key + "/mask"] = mask
            out[key + "/meta"] = np.frombuffer(json.dumps({"roi_begin": roi_begin, "chunk": chunk, "nhood": nhood,
                                                          "thresholds": thresholds}).encode(), np.uint8)
            out[key + "/error_map"] = np.asarray(maps[0].data, np.uint8)
            out[key + "/error_mask"] = np.asarray(masks[0].data, np.uint8)
    for i, case in enumerate(VOI_CASES):
        gt, seg = make_voi_case(*case)
        report = rand_voi(gt, seg, return_cluster_scores=False)
        out[f"voi{i}/gt"], out[f"voi{i}/seg"] = gt, seg
        out[f"voi{i}/report"] = np.frombuffer(json.dumps({k: float(v) for k, v in report.items()
                                                           if k not in ("voi_split_i", "voi_merge_j")}).encode(), np.uint8)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): {len(ERROR_CASES)} error-map cases, {len(VOI_CASES)} rand_voi cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
