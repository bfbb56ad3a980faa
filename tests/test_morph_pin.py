"""The pin for what `bs refine morph` restates (tests/morph_ref.py): fastmorph's multilabel dilate (background_only, the mode
with its tie rule), erode (erode_border) and fill_holes_v2 (fix_borders, merge_threshold=0.95).  fastmorph is not installed here,
so this file REPORTS the parity as unpinned -- a skip with that reason -- until someone runs tools/gen_goldens_morph.py where it
is and commits tests/golden/morph_cases.npz; then the same test holds the restatement (and through it the kernels, bit-equal to
it in tests/test_morph_gpu.py) to the reference's `_apply_morph`.  CPU only."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import morph_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "morph_cases.npz")
UNPINNED = ("parity UNPINNED: tests/golden/morph_cases.npz is absent (fastmorph is not installed here); "
            "run tools/gen_goldens_morph.py where it is and commit the file")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_goldens_morph", os.path.join(ROOT, "tools", "gen_goldens_morph.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generator_says_what_is_missing_and_its_cases_cover_the_choices():
    gen = _gen()
    if importlib.util.find_spec("fastmorph") is None:
        before = os.path.exists(GOLD)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_goldens_morph.py")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "not installed here" in r.stdout and os.path.exists(GOLD) == before
    ops, forms, changed = set(), set(), {}
    for name, kind, args, op, iterations, xy in gen.CASES:
        a = gen.make_case(kind, args)
        assert np.array_equal(a, gen.make_case(kind, args)) and a.dtype == np.uint64 and a.ndim == 3
        ops.add(op)
        forms.add(xy)
        changed[name] = not np.array_equal(R.apply_block(a, op, iterations, xy), a)
    assert ops == {"dilate", "erode", "opening", "closing", "fill_holes"} and forms == {False, True}
    by = {c[0]: c for c in gen.CASES}
    # ties between ids, touching labels, holes at 94 % and 96 % contact, holes cut by the array's face
    assert sum(R.tied_voxels(s) for s in gen.make_case("ties", ())) >= 3
    cells = gen.make_case(*by["dilate3d"][1:3])
    assert R.tied_voxels(cells) > 0 and ((cells[:, :, 1:] != cells[:, :, :-1]) & (cells[:, :, 1:] != 0) & (cells[:, :, :-1] != 0)).any()
    assert not changed["fill94"] and changed["fill96"] and changed["fill_face"] and changed["fill_face2d"]
    face = gen.make_case("face", ())
    assert (R.fill_holes(face)[3, 4, 0:3] == 0).all() and R.fill_holes(face)[3, 4, 8] == 4
    assert all(changed[n] for n in changed if not n.startswith("fill9"))


def test_restatement_against_reference_goldens():
    if not os.path.exists(GOLD):
        pytest.skip(UNPINNED)
    g = np.load(GOLD)
    names = sorted({k.split("/")[0] for k in g.files})
    assert names
    for name in names:
        meta = json.loads(bytes(g[name + "/meta"]).decode())
        got = R.apply_block(g[name + "/in"], meta["op"], meta["iterations"], meta["xy"])
        assert np.array_equal(got, g[name + "/out"]), (name, int((got != g[name + "/out"]).sum()))
