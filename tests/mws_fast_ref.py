"""Vectorised restatement of the mutex watershed for product-sized cases -- TEST INFRASTRUCTURE ONLY.

oracle/mws_ref.py lists and orders the edges with python loops, which holds it to a few thousand voxels.  The costly part
is that listing and ordering, not the sweep, so this module lists the edges with array operations, orders them with
`np.argsort(-|w|, kind="stable")` and hands them to the oracle's own sweep (`mws_ref._Forest`, a dict-of-sets union-find
whose clusters hold the set of roots they must stay apart from -- deliberately another representation than the library's
sorted lists of constraint ids).  tests/test_mws_fast_ref_cpu.py holds both functions equal to the oracle on small cases.

Plain numpy; nothing of the package under test is imported here.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.mws_ref import _Forest  # noqa: E402


def in_bounds(shape, offset):
    """bool [D][H][W]: voxels p whose partner p + offset lies inside the volume."""
    m = np.ones(shape, dtype=bool)
    for ax, o in enumerate(int(v) for v in offset):
        idx = np.arange(shape[ax]) + o
        sel = [None, None, None]
        sel[ax] = slice(None)
        m &= ((idx >= 0) & (idx < shape[ax]))[tuple(sel)]
    return m


def _linear(shape, offset):
    return (int(offset[0]) * shape[1] + int(offset[1])) * shape[2] + int(offset[2])


def grid_edges(affs, offsets, strides=None, keep=None):
    """(k, p, q, w) arrays of the real edges in (k, p) ascending order.  A candidate (k, p) is real if p + offset_k is inside
    the volume on all three axes, if it passes the stride rule (all coordinates of p divisible by stride_k) -- or, where `keep`
    is given, if keep[k][p] is set -- and if |w| > 0 (NaN compares false: no edge)."""
    affs = np.asarray(affs, dtype=np.float64)
    K = affs.shape[0]
    shape = tuple(affs.shape[1:])
    ks, ps, qs, ws = [], [], [], []
    for k in range(K):
        m = in_bounds(shape, offsets[k])
        if keep is not None:
            m &= np.asarray(keep[k], dtype=bool).reshape(shape)
        elif strides is not None:
            for ax in range(3):
                sel = [None, None, None]
                sel[ax] = slice(None)
                m &= (np.arange(shape[ax]) % int(strides[k][ax]) == 0)[tuple(sel)]
        p = np.flatnonzero(m.ravel())  # ascending
        w = affs[k].ravel()[p]
        with np.errstate(invalid="ignore"):
            real = np.abs(w) > 0
        p, w = p[real], w[real]
        ks.append(np.full(len(p), k, dtype=np.int64))
        ps.append(p)
        qs.append(p + _linear(shape, offsets[k]))
        ws.append(w)
    return np.concatenate(ks), np.concatenate(ps), np.concatenate(qs), np.concatenate(ws)


def mws_agglom(affs, offsets, strides=None, keep=None):
    """labels u64 [D][H][W], the rule of oracle/mws_ref.py:mws_agglom (ties in (k, p) ascending order)."""
    affs = np.asarray(affs, dtype=np.float64)
    _, p, q, w = grid_edges(affs, offsets, strides, keep)
    order = np.argsort(-np.abs(w), kind="stable")
    f = _Forest(int(np.prod(affs.shape[1:])))
    edge = f.edge
    for u, v, x in zip(p[order].tolist(), q[order].tolist(), w[order].tolist()):
        edge(u, v, x)
    return f.labels().reshape(affs.shape[1:])


def pair_affinity(affs_u8, offsets, frags):
    """{(u, v): (sum of affinity bytes, count)}, the rule of oracle/mws_ref.py:pair_affinity."""
    affs_u8 = np.asarray(affs_u8)
    frags = np.asarray(frags)
    shape = tuple(frags.shape)
    ids, dense = np.unique(frags.ravel(), return_inverse=True)  # ids of any width: the pairs are packed from dense indices
    dense = dense.astype(np.int64).ravel()
    n = len(ids)
    zero = int(np.searchsorted(ids, 0)) if (ids == 0).any() else -1
    keys, vals = [], []
    for k in range(affs_u8.shape[0]):
        p = np.flatnonzero(in_bounds(shape, offsets[k]).ravel())
        a, b = dense[p], dense[p + _linear(shape, offsets[k])]
        m = (a != b) & (a != zero) & (b != zero)
        a, b, p = a[m], b[m], p[m]
        keys.append(np.minimum(a, b) * n + np.maximum(a, b))
        vals.append(affs_u8[k].ravel()[p].astype(np.int64))
    keys, vals = np.concatenate(keys), np.concatenate(vals)
    uniq, inv = np.unique(keys, return_inverse=True)
    counts = np.bincount(inv, minlength=len(uniq))
    sums = np.zeros(len(uniq), dtype=np.int64)  # integer accumulation (bincount's weights would sum in float64)
    np.add.at(sums, inv, vals)
    lo, hi = ids[uniq // n].tolist(), ids[uniq % n].tolist()
    return {(u, v): (s, c) for u, v, s, c in zip(lo, hi, sums.tolist(), counts.tolist())}
