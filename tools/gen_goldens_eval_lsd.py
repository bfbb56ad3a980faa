#!/usr/bin/env python3
"""One-command pin for the LSD form of `bs evaluate`: run this WHERE gunpowder, lsd (funkelab/lsd), funlib.persistence AND
the reference package `bootstrapper` ARE INSTALLED and commit the file it writes, tests/golden/eval_lsd_cases.npz.  From then
on tests/test_eval_lsd_pin.py holds tests/lsd_errors_ref.py (and oracle/lsd_ref.py inside it) -- and through them the HIP
kernels of csrc/eval.hip, which tests/test_evaluate_lsd_gpu.py holds to them stage by stage -- to the reference's own
`compute_errors(..., return_arrays=True)` on a `3d_lsds` dataset; until then that test reports "parity UNPINNED".

    python tools/gen_goldens_eval_lsd.py        # -> tests/golden/eval_lsd_cases.npz, or a clear "not installed" message

What the cases decide:
  * the region: descriptors, the normalising maximum and the morphology over the chunk grown by (2, 50, 50) voxels, or over
    the bare chunk.  The ROIs lie inside larger datasets and the chunks (8, 24, 24) are smaller than the margin, so the two
    readings differ on most voxels (over the bare chunk every chunk's first and last slice of error_mask would be empty);
  * lsd's LsdExtractor.get_descriptors against oracle/lsd_ref.py, thin objects and ids above 2^32 included;
  * the default sigma, the context and the zero padding of seg, pred and mask.
Inputs are made by numpy / scipy alone (seeded); the arrays stored are inputs and the reference's outputs -- data, not source.
"""
import json
import os
import sys
import tempfile

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "eval_lsd_cases.npz")
VOXEL_SIZE = (40, 8, 8)
CHUNK = (8, 24, 24)
# (seed, seg shape, ROI begin in seg, ROI shape, ROI begin in pred (and mask), voxels of pred after the ROI, masked, thresholds,
#  lsd_sigma or None for the default)
CASES = [
    (1, (30, 150, 160), (10, 60, 70), (10, 40, 44), (2, 30, 50), (2, 50, 20), False, (0.1, 1.0), None),
    (2, (30, 150, 160), (10, 60, 70), (10, 40, 44), (1, 3, 6), (2, 6, 4), True, (0.02, 0.6), None),
    (3, (12, 60, 80), (2, 20, 20), (8, 24, 40), (2, 20, 20), (2, 16, 20), True, (0.05, 1.0), 54),
]


def make_case(seed, seg_shape, roi_begin, roi_shape, pred_begin, pred_after, masked):
    """-> seg u64, pred u8 [10][...], mask u8 or None"""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    blobs = gaussian_filter(rng.random(seg_shape), (1, 4, 4))
    seg = (np.digitize(blobs, np.quantile(blobs, [0.2, 0.4, 0.6, 0.8])) + 1).astype(np.uint64)
    seg[:, :, seg_shape[2] // 2:] += np.uint64(7)
    seg[blobs < np.quantile(blobs, 0.1)] = 0
    b, s = roi_begin, roi_shape
    seg[b[0] + s[0] // 2, b[1] + 4:b[1] + s[1] - 4, b[2] + 3:b[2] + s[2] // 2] = 61            # a one-voxel-thick sheet
    for k in range(6):
        seg[b[0] + 1 + k, b[1] + 2 + 3 * k, b[2] + 5 + 5 * k] = 60                            # one-voxel objects
    seg[seg == 3] = np.uint64(2**32 + 5)
    seg[seg == 9] = np.uint64(2**63 + 1)
    pred_shape = [p + n + a for p, n, a in zip(pred_begin, roi_shape, pred_after)]
    noise = gaussian_filter(rng.random([10] + pred_shape), (0, 1, 5, 5))
    pred = ((noise - noise.min()) / (noise.max() - noise.min()) * 255).astype(np.uint8)
    mask = (rng.random(pred_shape) < 0.9).astype(np.uint8) if masked else None
    return seg, pred, mask


def main():
    missing = []
    for name in ("gunpowder", "lsd.train", "funlib.persistence", "bootstrapper.eval.compute_errors"):
        try:
            __import__(name)
        except ImportError as exc:
            missing.append(f"{name} ({exc})")
    if missing:
        print("not installed here: " + "; ".join(missing) + ".  Nothing written.  Run this script where the reference's "
              "evaluation stack is installed and commit tests/golden/eval_lsd_cases.npz.")
        return 2
    from funlib.persistence import prepare_ds
    from funlib.geometry import Coordinate
    from bootstrapper.eval.compute_errors import compute_errors

    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, (seed, seg_shape, roi_begin, roi_shape, pred_begin, pred_after, masked, thresholds, sigma) in enumerate(CASES):
            seg, pred, mask = make_case(seed, seg_shape, roi_begin, roi_shape, pred_begin, pred_after, masked)
            store = os.path.join(tmp, f"case{i}.zarr")
            vs = Coordinate(VOXEL_SIZE)

            def write(name, a, offset, chunks):
                ds = prepare_ds(os.path.join(store, name), shape=a.shape, offset=offset, voxel_size=vs, dtype=a.dtype, chunk_shape=chunks)
                ds[ds.roi] = a
                return os.path.join(store, name)

            pred_off = (Coordinate(roi_begin) - Coordinate(pred_begin)) * vs
            seg_path = write("seg", seg, Coordinate((0, 0, 0)), (8, 32, 32))
            pred_path = write("pred/3d_lsds", pred, pred_off, (10,) + CHUNK)
            mask_path = write("mask", mask, pred_off, (8, 32, 32)) if masked else None
            kwargs = {} if sigma is None else {"lsd_sigma": sigma}
            batch = compute_errors(seg_path, pred_path, mask_path, os.path.join(store, "out/error_map"),
                                   os.path.join(store, "out/error_mask"), thresholds=thresholds, roi_offset=Coordinate(roi_begin) * vs,
                                   roi_shape=Coordinate(roi_shape) * vs, return_arrays=True, **kwargs)
            maps = [a for k, a in batch.arrays.items() if "MAP" in str(k)]
            masks = [a for k, a in batch.arrays.items() if "ERROR_MASK" in str(k)]
            key = f"lsd{i}"
            out[key + "/seg"], out[key + "/pred"] = seg, pred
            if masked:
                out[key + "/mask"] = mask
            out[key + "/meta"] = np.frombuffer(json.dumps({"roi_begin": roi_begin, "roi_shape": roi_shape, "pred_begin": pred_begin,
                                                          "chunk": CHUNK, "voxel_size": VOXEL_SIZE, "thresholds": thresholds,
                                                          "sigma": sigma}).encode(), np.uint8)
            out[key + "/error_map"] = np.asarray(maps[0].data, np.uint8)
            out[key + "/error_mask"] = np.asarray(masks[0].data, np.uint8)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): {len(CASES)} LSD error-map cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
