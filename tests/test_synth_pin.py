"""The pin for what the synthetic-label source restates: skimage.morphology's star / disk / ellipse (the bitmaps of
bootstrapper_amd/synth_labels.py), skimage.measure.label's numbering and edt.edt (tests/synth_ref.py).  scikit-image and edt
are not installed here, so this file REPORTS the parity as unpinned -- a skip with that reason -- until someone runs
tools/gen_goldens_synth.py where they are and commits tests/golden/synth_pin.npz.  skimage's watershed is stored too, but the
device follows a rule of its own there: the test only counts how far the two partitions agree.  CPU only."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import synth_ref as R
from bootstrapper_amd import synth_labels as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "synth_pin.npz")
UNPINNED = ("parity UNPINNED: tests/golden/synth_pin.npz is absent (scikit-image and edt are not installed here); "
            "run tools/gen_goldens_synth.py where they are and commit the file")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_goldens_synth", os.path.join(ROOT, "tools", "gen_goldens_synth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generator_says_what_is_missing_and_covers_the_reference_draws():
    gen = _gen()
    if importlib.util.find_spec("skimage") is None or importlib.util.find_spec("edt") is None:
        before = os.path.exists(GOLD)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_goldens_synth.py")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "not installed here" in r.stdout and os.path.exists(GOLD) == before
    # create_labels.py draws star 2..8, disk 1..4, ellipse 2..4; obfuscate_labels.py star 2..8, disk 1..8, ellipse 2..8
    assert set(gen.STAR) == set(range(2, 9)) and set(gen.DISK) == set(range(1, 9)) and len(set(gen.ELLIPSE)) == 49
    for shape, seed in gen.FIELDS:
        binary, values, smooth = gen.field(shape, seed)
        assert binary.shape == values.shape == smooth.shape == shape and smooth.dtype == np.float32
        assert np.array_equal(binary, gen.field(shape, seed)[0]) and binary.any() and len(np.unique(values)) > 3


def test_restatement_against_reference_goldens():
    if not os.path.exists(GOLD):
        pytest.skip(UNPINNED)
    gen = _gen()
    g = np.load(GOLD)
    for a in gen.STAR:
        assert np.array_equal(S.star(a), g[f"star/{a}"]), a
    for r in gen.DISK:
        assert np.array_equal(S.disk(r), g[f"disk/{r}"]), r
    for w, h in gen.ELLIPSE:
        assert np.array_equal(S.ellipse(w, h), g[f"ellipse/{w}_{h}"]), (w, h)
    for k in (1, 2):
        assert np.array_equal(S.binary_structure(k), g[f"structure/{k}"])
    for i, (shape, seed) in enumerate(gen.FIELDS):
        binary, values, smooth = gen.field(shape, seed)
        assert np.array_equal(R.label(binary.astype(np.int32))[0], g[f"field{i}/label_binary"])
        assert np.array_equal(R.label(values)[0], g[f"field{i}/label_values"])
        assert np.array_equal(R.split_field(binary | (values % 3 == 0)), np.rint(g[f"field{i}/edt"].astype(np.float64) ** 2).astype(np.float32))
        ours = R.basins(smooth, R.argmax_filter(smooth, 5))[0]
        same = np.mean((ours[..., 1:] == ours[..., :-1]) == (g[f"field{i}/watershed"][..., 1:] == g[f"field{i}/watershed"][..., :-1]))
        print(f"field {i}: {ours.max()} basins, skimage {g[f'field{i}/watershed'].max()}; boundaries along x agree on {same:.3f} of the pairs")
