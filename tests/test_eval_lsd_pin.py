"""The pin for what the LSD form of `bs evaluate` restates (tests/lsd_errors_ref.py, oracle/lsd_ref.py): the region each chunk is
processed over, lsd's descriptors, the default sigma and context, the padding, the f32 order of AddLSDErrors._create_diff and its
morphology.  gunpowder and lsd are not installed here, so this file REPORTS the parity as unpinned -- a skip with that reason --
until someone runs tools/gen_goldens_eval_lsd.py where they are and commits tests/golden/eval_lsd_cases.npz.  CPU only."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lsd_errors_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "eval_lsd_cases.npz")
UNPINNED = ("parity UNPINNED: tests/golden/eval_lsd_cases.npz is absent (gunpowder / lsd are not installed here); "
            "run tools/gen_goldens_eval_lsd.py where they are and commit the file")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_goldens_eval_lsd", os.path.join(ROOT, "tools", "gen_goldens_eval_lsd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generator_says_what_is_missing_and_its_cases_show_the_region():
    gen = _gen()
    try:
        import gunpowder  # noqa: F401
        import lsd.train  # noqa: F401
        have = True
    except ImportError:
        have = False
    if not have:
        before = os.path.exists(GOLD)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_goldens_eval_lsd.py")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "not installed here" in r.stdout and os.path.exists(GOLD) == before
    masked, sigmas = set(), set()
    for seed, seg_shape, roi_begin, roi_shape, pred_begin, pred_after, m, thresholds, sigma in gen.CASES:
        seg, pred, mask = gen.make_case(seed, seg_shape, roi_begin, roi_shape, pred_begin, pred_after, m)
        seg2, pred2, _ = gen.make_case(seed, seg_shape, roi_begin, roi_shape, pred_begin, pred_after, m)
        assert np.array_equal(seg, seg2) and np.array_equal(pred, pred2) and (mask is not None) == m
        assert pred.shape[0] == 10 and pred.dtype == np.uint8 and (seg >= 2**32).any()
        # ROIs inside larger datasets, chunks smaller than the margin
        assert all(b > 0 and b + n < s for b, n, s in zip(roi_begin, roi_shape, seg_shape))
        assert all(c < mg for c, mg in zip(gen.CHUNK[1:], L.MARGIN[1:]))
        masked.add(m)
        sigmas.add(sigma)
    assert masked == {False, True} and None in sigmas and len(sigmas) > 1
    # the two readings of the region differ on the smallest case: over the bare chunk the mask's first slice is empty
    seed, seg_shape, roi_begin, roi_shape, pred_begin, pred_after, m, thresholds, sigma = gen.CASES[2]
    seg, pred, mask = gen.make_case(seed, seg_shape, roi_begin, roi_shape, pred_begin, pred_after, m)
    got = {}
    for margin in (L.MARGIN, (0, 0, 0)):
        got[margin] = L.lsd_errors(seg, roi_begin, pred, pred_begin, roi_shape, gen.CHUNK, sigma, gen.VOXEL_SIZE, thresholds, mask,
                                   pred_begin, margin)
    assert not got[(0, 0, 0)][1][0].any() and got[L.MARGIN][1][0].any()
    assert not np.array_equal(got[(0, 0, 0)][0], got[L.MARGIN][0])


def test_restatement_against_reference_goldens():
    """the lsd package keeps its coordinates in float32, the restatement in float64: error_map may differ by one grey level where
    d * 255 falls next to an integer, error_mask where d falls next to a threshold and the morphology keeps the voxel"""
    if not os.path.exists(GOLD):
        pytest.skip(UNPINNED)
    g = np.load(GOLD)
    names = sorted({k.split("/")[0] for k in g.files if k.startswith("lsd")})
    assert names
    for name in names:
        meta = json.loads(bytes(g[name + "/meta"]).decode())
        mask = g[name + "/mask"] if name + "/mask" in g.files else None
        sigma = meta["sigma"] if meta["sigma"] is not None else L.default_sigma(meta["voxel_size"])
        emap, emask = L.lsd_errors(g[name + "/seg"], meta["roi_begin"], g[name + "/pred"], meta["pred_begin"], meta["roi_shape"],
                                   meta["chunk"], sigma, meta["voxel_size"], meta["thresholds"], mask, meta["pred_begin"])
        want_map, want_mask = g[name + "/error_map"], g[name + "/error_mask"]
        delta = np.abs(emap.astype(np.int16) - want_map.astype(np.int16))
        assert delta.max() <= 1 and (delta != 0).mean() <= 0.01, (name, int(delta.max()), float((delta != 0).mean()))
        assert (emask != want_mask).mean() <= 1e-3, (name, float((emask != want_mask).mean()))
