#!/usr/bin/env python3
"""One-command pin for the synthetic-label source: run this WHERE scikit-image AND edt ARE INSTALLED and commit the file it
writes, tests/golden/synth_pin.npz.  From then on tests/test_synth_pin.py holds the restated structuring bitmaps of
bootstrapper_amd/synth_labels.py and the labelling and distance rules of tests/synth_ref.py -- and through it the HIP kernels
of csrc/synth.hip, which tests/test_synth_gpu.py holds bit-equal to it -- to the packages the reference calls; until then
that test reports "parity UNPINNED".

    python tools/gen_goldens_synth.py           # -> tests/golden/synth_pin.npz, or a clear "not installed" message

What is stored (data, not source): star / disk / ellipse / generate_binary_structure for every radius the reference draws
(gp/create_labels.py:107-115, gp/obfuscate_labels.py:119-124); on three small seeded fields skimage.measure.label of a
binary and of a many-valued volume, edt.edt of a mask, and skimage.segmentation.watershed as create_labels.py:163-167 calls
it (whose flood order the device does not restate: DESIGN.md section 7i)."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "synth_pin.npz")
STAR, DISK, ELLIPSE = range(2, 9), range(1, 9), [(w, h) for w in range(2, 9) for h in range(2, 9)]
FIELDS = [((6, 20, 22), 1), ((9, 17, 33), 2), ((1, 24, 24), 3)]


def field(shape, seed):
    """(binary, many-valued, smooth float32) volumes of one seed, numpy alone"""
    rng = np.random.default_rng(seed)
    binary = rng.random(shape) < 0.15
    z, y, x = np.indices(shape)
    values = ((y // 5) * 7 + x // 6 + 1) * (rng.random(shape) < 0.9)
    smooth = rng.random(shape).astype(np.float32)
    for ax in range(3):
        smooth = (smooth + np.roll(smooth, 1, ax) + np.roll(smooth, -1, ax)) / np.float32(3)
    return binary, values.astype(np.int32), smooth


def main():
    missing = [m for m in ("skimage", "edt", "scipy") if importlib.util.find_spec(m) is None]
    if missing:
        print(f"{', '.join(missing)} not installed here: nothing written (tests/test_synth_pin.py keeps reporting UNPINNED)")
        return 2
    import edt
    from scipy.ndimage import generate_binary_structure, label as nd_label, maximum_filter
    from skimage.measure import label
    from skimage.morphology import disk, ellipse, star
    from skimage.segmentation import watershed
    out = {}
    for a in STAR:
        out[f"star/{a}"] = star(a).astype(bool)
    for r in DISK:
        out[f"disk/{r}"] = disk(r).astype(bool)
    for w, h in ELLIPSE:
        out[f"ellipse/{w}_{h}"] = ellipse(w, h).astype(bool)
    for k in (1, 2):
        out[f"structure/{k}"] = generate_binary_structure(2, k)
    for i, (shape, seed) in enumerate(FIELDS):
        binary, values, smooth = field(shape, seed)
        out[f"field{i}/label_binary"] = label(binary).astype(np.int32)
        out[f"field{i}/label_values"] = label(values).astype(np.int32)
        out[f"field{i}/edt"] = edt.edt(binary | (values % 3 == 0)).astype(np.float32)
        seeds = label(maximum_filter(smooth, 5) == smooth, connectivity=1)
        out[f"field{i}/watershed"] = watershed(1.0 - smooth, seeds).astype(np.int32)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} arrays)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
