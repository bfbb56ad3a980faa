"""The vectorised mutex-watershed reference (tests/mws_fast_ref.py) against the naive restatement (oracle/mws_ref.py) on
small cases: what the scale tests on the device compare with is first held equal, label for label, to the loops it replaces."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mws_fast_ref as F  # noqa: E402
from oracle import mws_ref  # noqa: E402

MIXED = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, -3, 3], [2, 0, -2], [-1, 4, 0]]
NEG = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -3, 0], [0, 0, -3]]
BIAS = np.array([-0.4, -0.4, -0.4, -0.7, -0.7, -0.7]).reshape(-1, 1, 1, 1)


def _tied(shape, seed, k=6, levels=9):
    """few distinct values of both signs: nearly every decision of the sweep rests on the tie order"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, levels, size=(k,) + tuple(shape)).astype(np.float64) / (levels - 1) + BIAS[:k]


def _naive_keep(affs, offsets, keep):
    """mws_ref.mws_agglom with an explicit mask in place of the stride rule (the naive listing, filtered)"""
    edges = [e for e in mws_ref.grid_edges(affs, offsets) if abs(e[3]) > 0 and keep[e[0]].ravel()[e[1]]]
    order = sorted(range(len(edges)), key=lambda i: -abs(edges[i][3]))
    f = mws_ref._Forest(int(np.prod(affs.shape[1:])))
    for i in order:
        f.edge(edges[i][1], edges[i][2], edges[i][3])
    return f.labels().reshape(affs.shape[1:])


@pytest.mark.parametrize("shape,offsets,strides", [
    ((3, 7, 11), MIXED, None),
    ((5, 6, 7), MIXED, [[1, 1, 1], [1, 2, 1], [1, 1, 2], [1, 2, 2], [2, 1, 1], [1, 3, 2]]),
    ((4, 6, 9), NEG, [[1, 1, 1]] * 3 + [[2, 3, 3]] * 3),
    ((1, 9, 10), MIXED, None),                                  # [2, 0, -2] is longer than the extent: that channel has no edge
    ((2, 5, 6), MIXED + [[0, 0, 6], [0, -5, 0], [-2, 0, 0]], None),   # offsets as long as the extent on each axis
    ((4, 5, 6), [[0, -2, 3]], None),                            # K = 1
])
def test_agglom_equals_the_naive_restatement(shape, offsets, strides):
    a = _tied(shape, len(offsets) + shape[2], k=min(len(offsets), 6))
    if len(offsets) > 6:
        a = np.concatenate([a, a[:len(offsets) - 6] + 0.125])
    ref = mws_ref.mws_agglom(a, offsets, strides)
    got = F.mws_agglom(a, offsets, strides)
    assert got.dtype == np.uint64 and np.array_equal(got, ref)
    assert 1 < len(np.unique(ref)) < ref.size
    k, p, q, w = F.grid_edges(a, offsets, strides)
    naive = [e for e in mws_ref.grid_edges(a, offsets, strides) if abs(e[3]) > 0]
    assert list(zip(k.tolist(), p.tolist(), q.tolist(), w.tolist())) == naive   # the same edges in the same (k, p) order


def test_agglom_special_values():
    """zeros, -0.0, NaN: no edge; +-inf: the strongest edges; denormals: ordinary (weak) edges"""
    rng = np.random.default_rng(5)
    a = _tied((3, 6, 8), 5)
    flat = a.reshape(-1)
    idx = rng.permutation(flat.size)
    for j, v in enumerate([0.0, -0.0, np.nan, np.inf, -np.inf, 5e-324, -5e-324, 1e-310, -2e-310]):
        flat[idx[j * 40:(j + 1) * 40]] = v
    ref = mws_ref.mws_agglom(np.where(np.isnan(a), 0.0, a), MIXED)
    assert np.array_equal(F.mws_agglom(a, MIXED), ref)
    assert 1 < len(np.unique(ref)) < ref.size
    n = a[0].size
    assert np.array_equal(F.mws_agglom(np.zeros_like(a), MIXED).ravel(), np.arange(1, n + 1, dtype=np.uint64))
    assert np.array_equal(F.mws_agglom(np.full_like(a, np.nan), MIXED).ravel(), np.arange(1, n + 1, dtype=np.uint64))
    assert np.array_equal(F.mws_agglom(np.full_like(a, -0.3), MIXED).ravel(), np.arange(1, n + 1, dtype=np.uint64))
    assert (F.mws_agglom(np.full_like(a, 0.3), MIXED) == 1).all()


def test_agglom_with_a_keep_mask():
    shape = (3, 6, 7)
    a = _tied(shape, 9)
    strides = [[1, 1, 1], [1, 2, 1], [1, 1, 2], [1, 2, 2], [2, 1, 1], [1, 3, 2]]
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    grid = np.stack([(zz % s[0] == 0) & (yy % s[1] == 0) & (xx % s[2] == 0) for s in strides])
    assert np.array_equal(F.mws_agglom(a, MIXED, keep=grid), mws_ref.mws_agglom(a, MIXED, strides))   # the stride rule as a mask
    keep = np.random.default_rng(3).random((6,) + shape) < 0.4
    got = F.mws_agglom(a, MIXED, strides=strides, keep=keep)   # the mask takes the place of the stride rule
    assert np.array_equal(got, _naive_keep(a, MIXED, keep))
    assert not np.array_equal(got, mws_ref.mws_agglom(a, MIXED))


@pytest.mark.parametrize("shape,offsets", [
    ((3, 7, 11), MIXED),
    ((6, 10, 11), NEG),
    ((2, 5, 6), MIXED + [[0, 0, 6], [3, 0, 0]]),
    ((4, 5, 6), [[0, -2, 3]]),
])
def test_pair_affinity_equals_the_naive_restatement(shape, offsets):
    rng = np.random.default_rng(shape[1])
    frags = rng.integers(0, 9, size=shape).astype(np.uint64) * np.uint64(1 << 33) + np.uint64(3) * (rng.integers(0, 2, size=shape) > 0)
    frags[rng.random(shape) < 0.2] = 0
    affs = rng.integers(0, 256, size=(len(offsets),) + shape).astype(np.uint8)
    ref = mws_ref.pair_affinity(affs, offsets, frags)
    got = F.pair_affinity(affs, offsets, frags)
    assert len(ref) > 0 and got == ref
    assert all(type(s) is int and type(c) is int for s, c in got.values())
    assert F.pair_affinity(affs, offsets, np.zeros(shape, np.uint64)) == {}
    assert F.pair_affinity(affs, offsets, np.full(shape, 7, np.uint64)) == {}
