#!/usr/bin/env python3
"""One-command pin for `bs refine morph`: run this WHERE fastmorph, fastremap AND the reference package `bootstrapper` ARE
INSTALLED and commit the file it writes, tests/golden/morph_cases.npz.  From then on tests/test_morph_pin.py holds
tests/morph_ref.py -- and through it the HIP kernels of csrc/morph.hip, which tests/test_morph_gpu.py holds bit-equal to it -- to
the reference's own `_apply_morph` (refine.py:329-344); until then that test reports "parity UNPINNED".

    python tools/gen_goldens_morph.py           # -> tests/golden/morph_cases.npz, or a clear "not installed" message

What the cases decide (the restated choices of tests/morph_ref.py):
  * dilate: which id a background voxel takes between touching labels, ties between ids included, and that labelled voxels stay;
  * erode: labels eroding each other and the array's faces (erode_border);
  * fill_holes: holes whose faces lie 94 % and 96 % against one id, enclosed foreign ids, holes cut by the array's face, nested
    holes, and the 2-D form (fix_borders) against the 3-D one.
Inputs are made by numpy alone (seeded); the arrays stored are inputs and the reference's outputs -- data, not source.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "morph_cases.npz")
# (name, kind, arguments of the maker, op, iterations, per section)
CASES = [
    ("dilate3d", "cells", ((9, 40, 52), 30, 41), "dilate", 1, False),
    ("dilate3d_n3", "cells", ((9, 40, 52), 30, 41), "dilate", 3, False),
    ("dilate2d", "cells", ((3, 40, 52), 20, 42), "dilate", 2, True),
    ("erode3d", "cells", ((9, 40, 52), 30, 41), "erode", 1, False),
    ("erode2d_n2", "cells", ((3, 40, 52), 20, 42), "erode", 2, True),
    ("opening3d", "cells", ((9, 40, 52), 30, 43), "opening", 1, False),
    ("closing2d", "cells", ((3, 40, 52), 20, 44), "closing", 2, True),
    ("ties", "ties", (), "dilate", 1, True),
    ("fill94", "contact", (6,), "fill_holes", 1, False),
    ("fill96", "contact", (5,), "fill_holes", 1, False),
    ("fill3d", "holes", ((9, 40, 52), 45), "fill_holes", 1, False),
    ("fill2d", "holes", ((3, 40, 52), 46), "fill_holes", 1, True),
    ("fill_face", "face", (), "fill_holes", 1, False),
    ("fill_face2d", "face", (), "fill_holes", 1, True),
]


def make_case(kind, args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import morph_ref as R
    if kind == "cells":
        return R.cells(*args)
    if kind == "holes":
        return R.holes(*args)
    if kind == "contact":
        return R.contact_case(*args)
    if kind == "ties":            # two ids once each, two against one, and three ids level around one background voxel
        a = np.zeros((1, 7, 15), np.uint64)
        a[0, 0, 0:2], a[0, 2, 0] = 9, 4
        a[0, 0, 4], a[0, 2, 4] = 7, 3
        a[0, 4, 8], a[0, 4, 10], a[0, 6, 9] = 12, 11, 13
        return a
    if kind == "face":            # a cavity cut by the array's face, a closed one, a nested one, a foreign id
        a = np.full((7, 25, 25), 4, np.uint64)
        a[3, 4, 0:3] = 0
        a[3, 4, 8] = 0
        a[2:5, 10:20, 10:20] = 8
        a[3, 14, 14] = 0
        a[5, 6, 6] = 11
        return a
    raise ValueError(kind)


def main():
    missing = []
    for name in ("fastmorph", "fastremap", "bootstrapper.refine"):
        try:
            __import__(name)
        except ImportError as exc:
            missing.append(f"{name} ({exc})")
    if missing:
        print("not installed here: " + "; ".join(missing) + ".  Nothing written.  Run this script where fastmorph and the "
              "reference package are installed and commit tests/golden/morph_cases.npz.")
        return 2
    from bootstrapper.refine import _apply_morph

    out = {}
    for name, kind, args, op, iterations, xy in CASES:
        a = make_case(kind, args)
        if xy:                    # refine.py:351-354
            res = np.stack([_apply_morph(a[z], op, iterations) for z in range(a.shape[0])])
        else:
            res = _apply_morph(a, op, iterations)
        out[name + "/in"], out[name + "/out"] = a, np.asarray(res, np.uint64)
        out[name + "/meta"] = np.frombuffer(json.dumps({"op": op, "iterations": iterations, "xy": xy}).encode(), np.uint8)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): {len(CASES)} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
