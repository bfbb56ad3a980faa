"""`bs segment --mws` at the sizes and inputs the product runs, against the vectorised restatement (tests/mws_fast_ref.py, held
equal to oracle/mws_ref.py by tests/test_mws_fast_ref_cpu.py).  Labels are compared with np.array_equal throughout: the same
labelling rule (1 + smallest voxel index), not only the same partition.

Reference times in the comments are single runs of mws_fast_ref on the host (one core), noted so that a later change of a shape
knows what it costs; nothing here asserts a time.
"""
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mws_fast_ref as F  # noqa: E402
from oracle import mws_ref  # noqa: E402

NEG = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -3, 0], [0, 0, -3]]
# positive and mixed-sign entries: the upper half of the bound check decides where the lower half passes
MIXED = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, -3, 3], [2, 0, -2], [-1, 4, 0]]
BIAS = [-0.4, -0.4, -0.4, -0.7, -0.7, -0.7]


def _device_agglom(a, offsets, strides=None, randomized=False, seed=0):
    import torch
    from bootstrapper_amd.post.mws import mws_agglom
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    return mws_agglom(t, offsets, strides, randomized, seed).cpu().numpy().view(np.uint64)


def _device_pairs(affs_u8, offsets, frags_u64):
    import torch
    from bootstrapper_amd.post.watershed_mutex import pair_affinities
    a = affs_u8 if torch.is_tensor(affs_u8) else torch.from_numpy(np.ascontiguousarray(affs_u8)).cuda()
    return pair_affinities(a, offsets, torch.from_numpy(np.ascontiguousarray(frags_u64).view(np.int64)).cuda())


def _check_pairs(got, ref):
    """edges, mean and counts of pair_affinities against {(u, v): (sum, count)}: exactly"""
    e, mean, cnt = got
    keys = [tuple(r) for r in e.tolist()]
    assert len(keys) == len(ref) and len(set(keys)) == len(keys)
    rs = np.array([ref.get(k, (0, 0))[0] for k in keys], dtype=np.float64)
    rc = np.array([ref.get(k, (0, 0))[1] for k in keys], dtype=np.uint64)
    assert np.array_equal(cnt, rc)
    assert np.array_equal(mean, rs / rc.astype(np.float64) / 255.0)


def _smooth_u8(shape, k, seed):
    """smoothed noise as affinity bytes: neighbouring voxels are alike, the values fill 0..255"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((k,) + tuple(shape))
    for ax in (1, 2, 3, 2, 3):
        a = a + np.roll(a, 1, ax) + np.roll(a, -1, ax)
    a = a / a.std() * 0.22 + 0.5
    return np.clip(np.rint(a * 255.0), 0, 255).astype(np.uint8)


def _product_weights(shape, seed, bias):
    """what the product hands to the sweep: u8 affinities / 255 + a bias per channel -- a few hundred distinct |w|"""
    u8 = _smooth_u8(shape, len(bias), seed)
    return u8.astype(np.float64) / 255.0 + np.asarray(bias, dtype=np.float64).reshape(-1, 1, 1, 1)


# ---- a. the three algorithms of the device sort ----------------------------------------------------------------------------
# hipcub::DeviceRadixSort forwards to rocprim::radix_sort_pairs_desc, which picks its algorithm by the number of items
# (rocprim/device/device_radix_sort.hpp:613-644 of the installed rocPRIM; limits from device_radix_sort_config.hpp:50):
# one block up to 256 * 4 = 1024 items, a merge sort up to 1024 * 1024, onesweep above.  The candidate counts K * D * H * W below
# sit on both sides of both limits and well inside onesweep.  The limits belong to that library, so nothing here asserts them:
# every case only asks for the documented order, whichever algorithm made it.
# K = 1 gives chains, where no tie order can change the result (those two cases hold the pairing of keys and values at 1024 and
# 1025 items); the K = 4 / K = 5 cases at the same counts have cycles, and each asserts that its result changes when the ties are
# taken in reverse.
PLANE4 = [[0, -1, 0], [0, 0, -1], [0, -3, 0], [0, 0, -3]]
PLANE5 = [[0, -1, 0], [0, 0, -1], [0, -2, 0], [0, 0, -3], [0, -1, -2]]
VOL4 = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [0, -4, 4]]
VOL4_STRIDES = [[1, 2, 1], [1, 1, 2], [1, 2, 1], [1, 2, 2]]
NEG_STRIDES = [[1, 2, 1], [1, 1, 2], [1, 2, 1], [1, 2, 2], [1, 2, 2], [1, 2, 2]]
SORT_CASES = [
    # shape, seed, offsets, bias, strides                                         candidates  real edges  reference on the host
    ((1, 32, 32), 132, [[0, 0, -1]], [-0.4], None),                                 # 1,024       987         < 0.01 s
    ((1, 25, 41), 141, [[0, 0, -1]], [-0.4], None),                                 # 1,025       997         < 0.01 s
    ((1, 16, 16), 116, PLANE4, [-0.4, -0.4, -0.7, -0.7], None),                     # 1,024       893         < 0.01 s
    ((1, 5, 41), 7, PLANE5, [-0.4, -0.4, -0.7, -0.7, -0.7], None),                  # 1,025       828         < 0.01 s
    ((4, 256, 256), 356, VOL4, [-0.4, -0.4, -0.4, -0.7], VOL4_STRIDES),             # 1,048,576   420,638     2.3 s
    ((4, 256, 257), 357, VOL4, [-0.4, -0.4, -0.4, -0.7], VOL4_STRIDES),             # 1,052,672   423,062     2.5 s
    ((8, 160, 160), 260, NEG, BIAS, NEG_STRIDES),                                   # 1,228,800   429,525     1.9 s
]


def _with_ties_reversed(a, offsets, strides):
    """the sweep of mws_fast_ref.mws_agglom with every run of equal |w| taken in (k, p) DESCENDING order"""
    _, p, q, w = F.grid_edges(a, offsets, strides)
    order = len(w) - 1 - np.argsort(-np.abs(w[::-1]), kind="stable")
    f = mws_ref._Forest(a[0].size)
    for u, v, x in zip(p[order].tolist(), q[order].tolist(), w[order].tolist()):
        f.edge(u, v, x)
    return f.labels().reshape(a.shape[1:])


@pytest.mark.parametrize("shape,seed,offsets,bias,strides", SORT_CASES, ids=["x".join(map(str, c[0])) + f"-K{len(c[2])}" for c in SORT_CASES])
def test_sort_regimes(shape, seed, offsets, bias, strides):
    a = _product_weights(shape, seed, bias)
    n, K = int(np.prod(shape)), len(offsets)
    # what the case asserts about its own input, so that it cannot pass vacuously
    k, p, _, w = F.grid_edges(a, offsets, strides)
    if K * n >= 1 << 20:
        assert len(w) >= 100_000
    assert len(np.unique(np.abs(w))) <= 1000          # ties dominate
    for c in range(K):
        # real edges at both ends of every channel: in the first and in the last tenth of its in-bounds candidates (a tenth of
        # the voxels cannot be meant: it is less than one slice here, and an offset along z has no partner in the first or last)
        cand = np.flatnonzero(F.in_bounds(shape, offsets[c]).ravel())
        pc, t = p[k == c], max(1, len(cand) // 10)
        assert (pc <= cand[t - 1]).any() and (pc >= cand[-t]).any()
    t0 = time.perf_counter()
    ref = F.mws_agglom(a, offsets, strides)
    t1 = time.perf_counter()
    got = _device_agglom(a, offsets, strides)
    t2 = time.perf_counter()
    print(f"mws {shape} K={K}: {K * n} candidates, {len(w)} real edges, {len(np.unique(np.abs(w)))} distinct |w|, "
          f"{len(np.unique(ref))} segments; reference {t1 - t0:.2f} s, mws_agglom (upload, keys, sort, host sweep, labels back) {t2 - t1:.3f} s")
    assert 1 < len(np.unique(ref)) < n
    if 1 < K and K * n < 1 << 16:
        assert not np.array_equal(_with_ties_reversed(a, offsets, strides), ref)   # the tie order decides in this input (small cases: it doubles the reference)
    assert np.array_equal(got, ref)


# ---- b. offsets of both signs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 7, 11), (5, 12, 13)])
def test_mixed_sign_offsets(shape):
    import torch
    a = _product_weights(shape, 7 + shape[0], BIAS)
    ref = mws_ref.mws_agglom(a, MIXED)
    assert np.array_equal(F.mws_agglom(a, MIXED), ref) and 1 < len(np.unique(ref)) < ref.size
    assert np.array_equal(_device_agglom(a, MIXED), ref)
    # a non-contiguous view of the same values
    t = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 2, 1))).cuda().permute(0, 3, 2, 1)
    assert not t.is_contiguous() and tuple(t.shape) == a.shape
    assert np.array_equal(_device_agglom(t, MIXED), ref)
    # strides on top
    strides = [[1, 1, 1], [1, 2, 1], [1, 1, 2], [1, 2, 2], [2, 1, 1], [1, 3, 2]]
    assert np.array_equal(_device_agglom(a, MIXED, strides), mws_ref.mws_agglom(a, MIXED, strides))
    # channels whose offset exceeds the extent on one axis (either sign) give no edge: the labels of the six remain
    far = [[shape[0], 0, 0], [0, -shape[1], 0], [0, 0, shape[2] + 5], [-1, 0, -shape[2]]]
    b = np.concatenate([a, np.full((len(far),) + shape, 0.95)])
    assert np.array_equal(_device_agglom(b, MIXED + far), ref)
    assert (_device_agglom(b[6:], far).ravel() == np.arange(1, ref.size + 1, dtype=np.uint64)).all()
    # K = 1, every offset on its own
    for c, off in enumerate(MIXED):
        assert np.array_equal(_device_agglom(a[c:c + 1], [off]), mws_ref.mws_agglom(a[c:c + 1], [off])), off


@pytest.mark.parametrize("shape", [(3, 7, 11), (5, 12, 13)])
def test_pair_affinities_mixed_sign_offsets(shape):
    import torch
    rng = np.random.default_rng(shape[1])
    frags = rng.integers(0, 9, size=shape).astype(np.uint64) * np.uint64(1 << 33)
    offsets = MIXED + [[0, 0, shape[2]], [-shape[0], 0, 0]]
    affs = rng.integers(0, 256, size=(len(offsets),) + shape).astype(np.uint8)
    ref = mws_ref.pair_affinity(affs, offsets, frags)
    assert F.pair_affinity(affs, offsets, frags) == ref and len(ref) > 0
    _check_pairs(_device_pairs(affs, offsets, frags), ref)
    t = torch.from_numpy(np.ascontiguousarray(affs.transpose(0, 3, 2, 1))).cuda().permute(0, 3, 2, 1)
    assert not t.is_contiguous()
    _check_pairs(_device_pairs(t, offsets, frags), ref)
    _check_pairs(_device_pairs(affs[3:4], MIXED[3:4], frags), mws_ref.pair_affinity(affs[3:4], MIXED[3:4], frags))


# ---- c. special values ----------------------------------------------------------------------------------------------------
def test_special_values_on_the_device():
    """+-inf are the strongest edges (ties among them in (k, p) order), denormals ordinary weak edges in the order of their
    magnitude, 0, -0.0 and NaN no edges."""
    shape = (3, 7, 11)
    rng = np.random.default_rng(5)
    a = _product_weights(shape, 5, BIAS)
    flat = a.reshape(-1)
    idx = rng.permutation(flat.size)
    for j, v in enumerate([0.0, -0.0, np.nan, np.inf, -np.inf, 5e-324, -5e-324, 1e-310, -2e-310, 2.3e-308]):
        flat[idx[j * 60:(j + 1) * 60]] = v
    ref = mws_ref.mws_agglom(np.where(np.isnan(a), 0.0, a), MIXED)
    assert np.array_equal(F.mws_agglom(a, MIXED), ref) and 1 < len(np.unique(ref)) < ref.size
    assert np.array_equal(_device_agglom(a, MIXED), ref)
    # only special values: the denormals and the infinities alone decide
    b = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 5e-324, -5e-324, 1e-310, -2e-310, 1e-320])[rng.integers(0, 10, size=a.shape)]
    ref = mws_ref.mws_agglom(np.where(np.isnan(b), 0.0, b), MIXED)
    assert 1 < len(np.unique(ref)) < ref.size
    assert np.array_equal(_device_agglom(b, MIXED), ref)
    each = np.arange(1, a[0].size + 1, dtype=np.uint64).reshape(shape)
    for v in (0.0, -0.0, np.nan):
        assert np.array_equal(_device_agglom(np.full_like(a, v), MIXED), each), v           # no edge at all
    for v in (-0.3, -np.inf, -5e-324):
        assert np.array_equal(_device_agglom(np.full_like(a, v), MIXED), each), v           # all repulsive
    for v in (0.3, np.inf, 5e-324):
        assert (_device_agglom(np.full_like(a, v), MIXED) == 1).all(), v                    # all equal and attractive


# ---- d. constraints inherited over a long sweep ---------------------------------------------------------------------------
def _rows_case():
    H = W = 64
    rng = np.random.default_rng(2)
    a = np.zeros((4, 1, H, W))
    a[0] = 0.9 + 1e-3 * rng.permutation(H * W).reshape(1, H, W) / (H * W)   # distinct: their order is fixed, and scrambled
    a[1] = -0.5
    a[2] = 0.3
    a[3] = 0.1
    return a, [[0, 0, -1], [0, -1, 0], [0, -2, 0], [0, -1, 0]]


def test_constraints_inherited_over_a_long_sweep():
    """(1, 64, 64), by the rule alone.  Channel 0, [0, 0, -1], 0.9..0.901: the strongest edges, all attractive, nothing forbids
    them: every row becomes one cluster.  Channel 1, [0, -1, 0], -0.5: next; the first edge between rows y - 1 and y puts a
    constraint between the two row clusters, the other 63 find them separated already.  Channel 2, [0, -2, 0], +0.3: row y and
    row y - 2 hold no common constraint (each is barred only from its direct neighbours, and unions so far joined rows of one
    parity only), so they unite, and the union inherits the constraints of both: after this channel the even rows are one cluster,
    the odd rows another, and the 63 constraints of channel 1 all lie between these two.  Channel 3, [0, -1, 0], +0.1: every edge
    joins an even row to an odd one and is refused.  Labels: even rows 1 (voxel 0), odd rows 1 + W (first voxel of row 1)."""
    a, offsets = _rows_case()
    W = a.shape[3]
    want = np.where(np.arange(a.shape[2]) % 2 == 0, 1, 1 + W).astype(np.uint64).reshape(1, -1, 1) * np.ones((1, 1, W), np.uint64)
    assert np.array_equal(F.mws_agglom(a, offsets), want)
    assert np.array_equal(_device_agglom(a, offsets), want)
    # without the repulsion the weakest channel is accepted: one segment (the refusals above are the constraints' doing)
    a[1] = 0.0
    assert (_device_agglom(a, offsets) == 1).all()


# ---- e. randomized strides ------------------------------------------------------------------------------------------------
RS_SHAPE = (7, 30, 31)
RS_STRIDES = [[1, 1, 1], [1, 1, 2], [1, 2, 1], [1, 2, 2], [2, 1, 1], [1, 3, 1]]


def _observe_kept(seed):
    """bool [K][D][H][W]: the candidates the device kept for (RS_STRIDES, seed).  The selection hashes (seed, edge index) and
    does not look at the weights.  With one channel uniformly attractive and all others zero the kept edges of that channel
    are the whole graph, a union of chains along the channel's offset: p and p + offset share a label exactly when the edge
    between them was kept."""
    kept = np.zeros((len(MIXED),) + RS_SHAPE, dtype=bool)
    for k, off in enumerate(MIXED):
        a = np.zeros((len(MIXED),) + RS_SHAPE)
        a[k] = 0.5
        lab = _device_agglom(a, MIXED, RS_STRIDES, True, seed).ravel()
        p = np.flatnonzero(F.in_bounds(RS_SHAPE, off).ravel())
        q = p + (off[0] * RS_SHAPE[1] + off[1]) * RS_SHAPE[2] + off[2]
        kept[k].reshape(-1)[p] = lab[p] == lab[q]
    return kept


def test_randomized_strides():
    kept = _observe_kept(3)
    for k, off in enumerate(MIXED):
        n = int(F.in_bounds(RS_SHAPE, off).sum())
        pr = 1.0 / np.prod(RS_STRIDES[k])
        got = int(kept[k].sum())
        print(f"randomized strides {RS_STRIDES[k]}: kept {got} of {n} in-bounds candidates, expected {n * pr:.0f} +- {np.sqrt(n * pr * (1 - pr)):.1f}")
        assert abs(got - n * pr) <= 5.0 * np.sqrt(n * pr * (1.0 - pr))   # binomial; a stride volume of 1 keeps everything (sd 0)
    assert kept[0].sum() == F.in_bounds(RS_SHAPE, MIXED[0]).sum()
    assert np.array_equal(_observe_kept(3), kept)                          # the same seed: the identical selection
    other = _observe_kept(4)
    assert all(not np.array_equal(other[k], kept[k]) for k in range(1, len(MIXED)))   # another seed: another one, in every thinned channel
    # the selection observed, the sweep over it is the restatement's with that mask: mixed-sign, tie-rich weights, same seed
    a = _product_weights(RS_SHAPE, 21, BIAS)
    ref = F.mws_agglom(a, MIXED, keep=kept)
    got = _device_agglom(a, MIXED, RS_STRIDES, True, 3)
    assert np.array_equal(got, ref) and 1 < len(np.unique(ref)) < ref.size
    assert not np.array_equal(ref, F.mws_agglom(a, MIXED, RS_STRIDES))      # ... and not the regular stride grid
    assert np.array_equal(_device_agglom(a, MIXED, [[1, 1, 1]] * 6, True, 3), F.mws_agglom(a, MIXED))


# ---- f. pair affinities at scale ------------------------------------------------------------------------------------------
def _blob_fragments(shape, seed):
    """wavy cells of about 2 x 8 x 8 voxels, one id each: ids beyond 2^32, and a sixth of the cells background (0)"""
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    cy = (yy + np.rint(3 * np.sin(xx / 7.0 + zz))).astype(np.int64) // 8 + 1
    cx = (xx + np.rint(3 * np.cos(yy / 5.0 - zz))).astype(np.int64) // 8 + 1
    cell = ((zz // 2) * 64 + cy) * 64 + cx
    ids = rng.permutation(1 << 16).astype(np.uint64) * np.uint64(1 << 33) + np.uint64(1)
    ids[rng.random(len(ids)) < 1.0 / 6.0] = 0
    return ids[cell]


def test_pair_affinities_at_scale():
    shape = (8, 160, 160)                       # 1,228,800 candidates; reference 0.05 s on the host
    frags = _blob_fragments(shape, 1)
    affs = _smooth_u8(shape, 6, 2)
    ref = F.pair_affinity(affs, MIXED, frags)
    assert (frags == 0).any() and int(frags.max()) > 1 << 32 and len(np.unique(frags)) > 1000 and len(ref) > 5000
    _check_pairs(_device_pairs(affs, MIXED, frags), ref)


def test_pair_affinity_sum_beyond_24_bits():
    """two ids alternating from slice to slice, every affinity 255: one pair, and its sum passes 2^24 (where a float32
    accumulator would stop counting exactly)"""
    shape = (8, 160, 160)
    u, v = (1 << 40) + 5, (1 << 33) + 1
    frags = np.where(np.arange(shape[0]) % 2 == 0, u, v).astype(np.uint64).reshape(-1, 1, 1) * np.ones(shape, np.uint64)
    affs = np.full((6,) + shape, 255, np.uint8)
    ref = F.pair_affinity(affs, MIXED, frags)
    pairs = 7 * 160 * 160 + 7 * 156 * 160       # [1, 0, 0] and [-1, 4, 0]; [2, 0, -2] stays within one id
    assert ref == {(v, u): (255 * pairs, pairs)} and 255 * pairs > 1 << 24
    _check_pairs(_device_pairs(affs, MIXED, frags), ref)


def test_pair_affinities_grow_their_capacity():
    """200 ids scattered voxel by voxel: nearly all of the 19,900 possible pairs occur, more than the first capacity of
    max(1024, 64 * 200) = 12,800, so pair_affinities has to take its second round"""
    shape = (6, 40, 40)
    rng = np.random.default_rng(4)
    frags = (rng.integers(1, 201, size=shape).astype(np.uint64)) * np.uint64(1 << 33)
    affs = rng.integers(0, 256, size=(6,) + shape).astype(np.uint8)
    ref = F.pair_affinity(affs, MIXED, frags)
    n = len(np.unique(frags))
    assert n == 200 and len(ref) > max(1024, 64 * n)
    _check_pairs(_device_pairs(affs, MIXED, frags), ref)
