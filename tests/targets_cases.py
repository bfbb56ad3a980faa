"""Fixtures of the training-target tests (test_targets_cpu.py, test_targets_gpu.py): pure numpy builders of label arrays at
the geometries where the target kernels can go wrong unseen, the references composed from the oracles, the faults a
kernel could have (restated on the reference) and the gates both modules hold results to.

Every builder returns a case: labels, the unlabelled mask (or None), the arguments of the device entry and a short name.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

# ---- gates (the project's: bit-equal labels / affinities / masks / tables, rtol 1e-6 on balance weights, 1e-4 on descriptors)
LSD_ATOL = 1e-4
BALANCE_RTOL = 1e-6


def gate_lsd(got, got_w, ref, ref_w, labels_roi):
    """descriptors to 1e-4 per channel, background exactly 0, weights bit-equal; -> largest error per channel"""
    assert got.shape == ref.shape and got.dtype == np.float32
    axes = tuple(range(1, got.ndim))
    err = np.abs(got.astype(np.float64) - ref).max(axis=axes)
    assert err.max() < LSD_ATOL, err
    assert (got[:, labels_roi == 0] == 0).all(), "background voxels must be exactly 0"
    if got_w is not None:
        assert np.array_equal(got_w, ref_w), "LSD weights"
    return err


def gate_affinity(got_grown, got_affs, got_weights, ref):
    assert np.array_equal(got_grown, ref["grown"]), "grown labels"
    assert np.array_equal(got_affs, ref["affs"]), "affinities"
    assert (got_weights[ref["mask"] == 0] == 0).all(), "weights must be exactly 0 where the mask is 0"
    assert np.isfinite(got_weights).all()
    assert np.allclose(got_weights, ref["weights"], rtol=BALANCE_RTOL, atol=0), "balance weights"


def gate_sat(got, ref):
    assert np.array_equal(got, ref), "summed-area table"


# ---- label makers ---------------------------------------------------------------------------------------------------
def voronoi(rng, shape, n_seeds, scale=None):
    """labels 1..n_seeds: nearest of n_seeds random seeds (blobs several voxels thick)"""
    scale = scale or (1,) * len(shape)
    seeds = rng.integers(0, shape, size=(n_seeds, len(shape)))
    grids = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    dist = sum(((g[..., None] - seeds[:, i]) * scale[i]) ** 2 for i, g in enumerate(grids))
    return (dist.argmin(-1) + 1).astype(np.int64)


def confetti(rng, shape, block, n_labels):
    """random labels 0..n_labels-1 (0 = background) in blocks of `block` voxels: many labels in every sub-grid cell"""
    small = rng.integers(0, n_labels, size=[-(-n // b) for n, b in zip(shape, block)]).astype(np.int64)
    for ax, b in enumerate(block):
        small = np.repeat(small, b, axis=ax)
    return np.ascontiguousarray(small[tuple(slice(0, n) for n in shape)]) * 1000003


# values that differ only above bit 31: every one is 1 modulo 2^32
HIGH = np.array([0] + [1 + h for h in [0, 1 << 32, 1 << 33, 1 << 62, 3 << 32, (1 << 62) + (1 << 32), 5 << 32] + [1 << b for b in range(34, 62)]],
                dtype=np.int64)


def highbits(labels):
    """labels 0..35 -> {0, 1, 1 + 2^32, 1 + 2^33, 2^62 + 1, ...}"""
    assert labels.max() < len(HIGH)
    return HIGH[labels]


def known_mask(rng, shape, frac=0.1):
    return (rng.random(shape) > frac).astype(np.uint8)


# ---- local shape descriptors ----------------------------------------------------------------------------------------
class LsdCase(NamedTuple):
    name: str
    labels: np.ndarray            # 3-D: [D][H][W]; 2-D: [S][H][W]
    unl: Optional[np.ndarray]
    roi_offset: tuple
    roi_shape: tuple
    sigma: tuple
    voxel_size: tuple
    df: int

    @property
    def roi(self):
        lead = (slice(None),) * (self.labels.ndim - len(self.roi_shape))
        return lead + tuple(slice(o, o + s) for o, s in zip(self.roi_offset, self.roi_shape))


def _thin3d():
    """filler label 1; a plane, rows and columns one voxel thick at odd coordinates (never on labels[::2]); label 10 has
    taps on the sub-grid, but only far from its thin part"""
    lab = np.ones((8, 28, 28), np.int64)
    lab[:, 3, :] = 2
    lab[:, 17, :] = 3
    lab[3, 9, :] = 4
    lab[5, 21, :] = 5
    lab[:, 7, 5] = 6
    lab[:, 19, 19] = 7
    lab[1, :, 11] = 8
    lab[5, :, 15] = 9
    lab[:, 24:, 24:] = 10
    lab[3, 1, :4] = 10
    return lab


def _thin2d():
    lab = np.ones((3, 40, 40), np.int64)
    for s in range(3):
        lab[s, 3 + 2 * s, :] = 2
        lab[s, 25 + 2 * s, :] = 3
        lab[s, :, 5 + 2 * s] = 4
        lab[s, :, 27 + 2 * s] = 5
        k = np.arange(1, 40, 2)
        lab[s, k, (k + 10 + 2 * s) % 40] = 6
        lab[s, 36:, 36:] = 10
        lab[s, 1, :3] = 10
    return lab


def _lsd3d(name):
    rng = np.random.default_rng(sum(name.encode()))
    if name in ("thin_origin", "thin_offset", "none"):
        lab = _thin3d()
        off = (0, 0, 0) if name == "thin_origin" else (2, 12, 12)
        return LsdCase(name, lab, None if name == "none" else known_mask(rng, lab.shape), off, (6, 16, 16), (10.0, 12.0, 9.0), (2.0, 2.0, 3.0), 2)
    if name == "highbits":
        lab = voronoi(rng, (8, 40, 40), 20, (4, 1, 1))
        lab[np.isin(lab, [3, 7])] = 0
        return LsdCase(name, highbits(lab), known_mask(rng, lab.shape), (2, 8, 8), (4, 24, 24), (10.0, 12.0, 9.0), (2.0, 2.0, 3.0), 2)
    if name == "edge":
        lab = voronoi(rng, (6, 20, 24), 12, (3, 1, 1)) * 1000003
        lab[lab == 5 * 1000003] = 0
        return LsdCase(name, lab, known_mask(rng, lab.shape), (0, 0, 0), lab.shape, (6.0, 6.0, 6.0), (3.0, 2.0, 2.0), 1)
    if name == "df4":
        lab = confetti(rng, (8, 48, 48), (1, 2, 2), 7)
        return LsdCase(name, lab, known_mask(rng, lab.shape), (0, 8, 4), (8, 32, 40), (12.0, 16.0, 20.0), (2.0, 2.0, 2.0), 4)
    if name == "df8":
        lab = confetti(rng, (8, 48, 64), (2, 2, 2), 7)
        return LsdCase(name, lab, known_mask(rng, lab.shape), (0, 8, 8), (8, 32, 48), (24.0, 40.0, 40.0), (2.0, 2.0, 2.0), 8)
    raise KeyError(name)


def _lsd2d(name):
    rng = np.random.default_rng(sum(name.encode()) + 1000)
    if name in ("thin_origin", "thin_offset", "none"):
        lab = _thin2d()
        off = (0, 0) if name == "thin_origin" else (16, 16)
        return LsdCase(name, lab, None if name == "none" else known_mask(rng, lab.shape), off, (24, 24), (10.0, 12.0), (2.0, 3.0), 2)
    if name == "highbits":
        lab = np.stack([voronoi(rng, (56, 60), 20) for _ in range(2)])
        lab[np.isin(lab, [3, 7])] = 0
        return LsdCase(name, highbits(lab), known_mask(rng, lab.shape), (16, 12), (24, 36), (10.0, 12.0), (2.0, 3.0), 2)
    if name == "edge":
        lab = np.stack([voronoi(rng, (24, 40), 10) for _ in range(2)]) * 1000003
        lab[lab == 4 * 1000003] = 0
        return LsdCase(name, lab, known_mask(rng, lab.shape), (0, 0), (24, 40), (6.0, 6.0), (2.0, 2.0), 1)
    if name == "df4":     # ROI of 16 x 20 cells: one tile in y, a full and a partial one in x
        lab = confetti(rng, (2, 128, 120), (1, 2, 2), 7)
        return LsdCase(name, lab, known_mask(rng, lab.shape), (32, 20), (64, 80), (40.0, 24.0), (4.0, 4.0), 4)
    if name == "df8":     # ROI of 20 x 16 cells
        lab = confetti(rng, (2, 192, 160), (1, 2, 2), 7)
        return LsdCase(name, lab, known_mask(rng, lab.shape), (16, 16), (160, 128), (80.0, 48.0), (4.0, 4.0), 8)
    if name == "rmax":    # r = 60 on both axes: the largest window the kernel accepts, 149 420 B of LDS
        lab = np.stack([voronoi(rng, (152, 160), 30) for _ in range(2)]) * 1000003
        lab[np.isin(lab // 1000003, [2, 9])] = 0
        return LsdCase(name, lab, known_mask(rng, lab.shape), (60, 60), (32, 40), (80.0, 80.0), (4.0, 4.0), 1)
    raise KeyError(name)


LSD3D_NAMES = ("thin_origin", "thin_offset", "highbits", "edge", "df4", "df8", "none")
LSD2D_NAMES = ("thin_origin", "thin_offset", "highbits", "edge", "df4", "df8", "rmax", "none")


@functools.lru_cache(maxsize=None)
def lsd_case(nd, name):
    return (_lsd3d if nd == 3 else _lsd2d)(name)


@functools.lru_cache(maxsize=None)
def lsd_reference(nd, name):
    """(descriptors float32, weights float32) of the scipy restatement: oracle/lsd_ref.py in 3-D, tests/lsd2d_ref.py in 2-D"""
    c = lsd_case(nd, name)
    if nd == 3:
        from oracle.lsd_ref import lsd_targets
    else:
        from lsd2d_ref import lsd2d_targets as lsd_targets
    ref, w = lsd_targets(c.labels, c.roi_offset, c.roi_shape, c.sigma, c.voxel_size, c.df, c.unl)
    ref.setflags(write=False)
    w.setflags(write=False)
    return ref, w


@functools.lru_cache(maxsize=None)
def lsd_direct_reference(nd, name, fault=None):
    """float64 descriptors of the direct sum (tests/lsd_direct_ref.py)"""
    from lsd_direct_ref import lsd_direct, lsd_direct_sections
    c = lsd_case(nd, name)
    out = (lsd_direct if nd == 3 else lsd_direct_sections)(c.labels, c.roi_offset, c.roi_shape, c.sigma, c.voxel_size, c.df, fault)
    out.setflags(write=False)
    return out


def cells_with_labels(case, at_least):
    """number of sub-grid cells of the ROI whose voxels hold `at_least` or more distinct labels (background counts)"""
    lab = case.labels[case.roi]
    df = case.df
    sp = lab.shape[-len(case.roi_shape):]
    lead = lab.shape[:lab.ndim - len(sp)]
    split = lab.reshape(lead + tuple(v for n in sp for v in (n // df, df)))
    nl = len(lead)
    cell_axes = [nl + 2 * i for i in range(len(sp))]
    vox_axes = [nl + 2 * i + 1 for i in range(len(sp))]
    cells = split.transpose(list(range(nl)) + cell_axes + vox_axes).reshape(-1, df ** len(sp))
    cells = np.sort(cells, axis=1)
    return int(((np.diff(cells, axis=1) != 0).sum(axis=1) + 1 >= at_least).sum())


# ---- affinities -----------------------------------------------------------------------------------------------------
PRODUCT9 = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -9, 0], [0, 0, -9], [-3, 0, 0], [0, -27, 0], [0, 0, -27]]
MIXED = [[1, 0, 0], [0, 3, -3], [0, -3, 3], [-1, 2, 0]]
MIXED16 = MIXED + [[0, 1, 0], [0, 0, 1], [2, 0, 0], [0, -2, 1], [1, 1, 1], [-1, -1, -1], [0, 3, 0], [0, 0, -3], [-2, 1, -1], [1, -2, 2], [0, 2, 2], [3, 0, 0]]
SECTION6 = [[0, -1, 0], [0, 0, -1], [0, -9, 0], [0, 0, -9], [0, -27, 0], [0, 0, -27]]
STACK6 = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 0, 0], [0, -3, 0], [0, 0, -3]]
GRID_CAP = 4096 * 256            # ROI voxels per sample that one pass of affinity_roi_kernel's grid covers


class AffCase(NamedTuple):
    name: str
    labels: np.ndarray            # whole-array entry: [D][H][W]; ROI entry: [S][D][H][W]
    unl: Optional[np.ndarray]
    nhood: list
    steps: int
    only_xy: bool
    roi_offset: Optional[tuple] = None   # None: the whole-array entry (affinity_targets)
    roi_shape: Optional[tuple] = None


def _patches(unl):
    """unknown regions that still carry labels"""
    unl[..., 5:12, 14:24] = 0
    unl[..., -2:, 20:, :6] = 0
    return unl


def _aff(name):
    rng = np.random.default_rng(sum(name.encode()) + 2000)
    if name in ("product9", "none"):
        lab = voronoi(rng, (6, 32, 34), 18, (4, 1, 1)) * 1000003
        lab[np.isin(lab // 1000003, [3, 7, 11])] = 0
        if name == "none":
            return AffCase(name, lab, None, PRODUCT9, 2, False)
        return AffCase(name, lab, _patches((lab > 0).astype(np.uint8)), PRODUCT9, 1, True)
    if name in ("mixed", "mixed16"):
        lab = voronoi(rng, (5, 30, 33), 18, (3, 1, 1)) * 1000003
        lab[np.isin(lab // 1000003, [2, 9])] = 0
        unl = _patches(np.ones(lab.shape, np.uint8))
        return AffCase(name, lab, unl, MIXED, 1, False) if name == "mixed" else AffCase(name, lab, unl, MIXED16, 0, True)
    if name == "highbits":
        lab = voronoi(rng, (4, 30, 30), 16, (3, 1, 1))
        lab[lab == 5] = 0
        return AffCase(name, highbits(lab), np.ones(lab.shape, np.uint8), PRODUCT9[:6], 1, True)
    if name == "clip_low":      # every voxel its own label: no positives
        lab = (np.arange(4 * 18 * 20, dtype=np.int64) + 1).reshape(4, 18, 20)
        return AffCase(name, lab, np.ones(lab.shape, np.uint8), PRODUCT9[:3], 0, True)
    if name == "clip_high":     # one label everywhere: no negatives
        lab = np.full((4, 18, 20), 5, np.int64)
        return AffCase(name, lab, np.ones(lab.shape, np.uint8), PRODUCT9[:3], 1, True)
    if name == "all_unknown":
        lab = voronoi(rng, (4, 18, 20), 8, (3, 1, 1))
        return AffCase(name, lab, np.zeros(lab.shape, np.uint8), PRODUCT9[:3], 1, True)
    raise KeyError(name)


def _aff_roi(name):
    rng = np.random.default_rng(sum(name.encode()) + 3000)
    if name == "product9":
        lab = np.stack([voronoi(rng, (6, 36, 38), 18, (4, 1, 1)) for _ in range(2)]) * 1000003
        lab[np.isin(lab // 1000003, [3, 7])] = 0
        return AffCase(name, lab, _patches((lab > 0).astype(np.uint8)), PRODUCT9, 1, True, (3, 27, 27), (3, 9, 11))
    if name in ("mixed", "none"):   # the ROI reaches the far faces: positive offsets leave the array
        lab = np.stack([voronoi(rng, (4, 24, 26), 12, (3, 1, 1)) for _ in range(2)]) * 1000003
        lab[np.isin(lab // 1000003, [2])] = 0
        if name == "none":
            return AffCase(name, lab, None, MIXED, 1, True, (1, 3, 3), (3, 21, 23))
        return AffCase(name, lab, _patches(np.ones(lab.shape, np.uint8)), MIXED, 1, False, (1, 3, 3), (3, 21, 23))
    if name == "highbits":
        lab = np.stack([voronoi(rng, (1, 40, 42), 16) for _ in range(2)])
        lab[lab == 5] = 0
        return AffCase(name, highbits(lab), np.ones(lab.shape, np.uint8), SECTION6, 1, True, (0, 27, 27), (1, 13, 15))
    if name == "regimes":       # section 0: clip_high, 1: clip_low, 2: all unknown, 3: mixed blobs
        shape = (1, 67, 71)
        lab = np.stack([np.full(shape, 5, np.int64), (np.arange(67 * 71, dtype=np.int64) + 1).reshape(shape),
                        voronoi(rng, shape, 12), voronoi(rng, shape, 12)])
        unl = np.ones(lab.shape, np.uint8)
        unl[2] = 0
        return AffCase(name, lab, unl, SECTION6, 1, True, (0, 27, 27), (1, 40, 44))
    if name in ("stack3d", "stack3d_xy"):
        # every sample is one 2-D pattern through all its sections, another in every sample: inside a sample no erosion crosses
        # sections, across a seam between samples every voxel would erode
        lab = np.stack([np.repeat(voronoi(rng, (1, 24, 26), 7), 5, axis=0) + 10 * s for s in range(3)])
        lab[1, 2, 8:12, 8:12] = 99                       # and one object that does erode along z
        unl = np.ones(lab.shape, np.uint8)
        unl[0, 4, :6, :] = 0
        unl[2, 0, 10:, 20:] = 0
        return AffCase(name, lab, unl, STACK6, 2, name == "stack3d_xy", (1, 3, 4), (4, 18, 20))
    if name == "stride":        # 1032 * 1024 ROI voxels per sample: the grid-stride loop of affinity_roi_kernel runs twice
        lab = confetti(rng, (2, 1, 1033, 1025), (1, 1, 8, 8), 6)
        unl = (lab > 0).astype(np.uint8)
        unl[1, 0, 500:, :300] = 0
        return AffCase(name, lab, unl, [[0, -1, 0], [0, 0, -1]], 0, True, (0, 1, 1), (1, 1032, 1024))
    raise KeyError(name)


AFF_NAMES = ("product9", "mixed", "mixed16", "highbits", "clip_low", "clip_high", "all_unknown", "none")
AFF_ROI_NAMES = ("product9", "mixed", "highbits", "none", "regimes", "stack3d", "stack3d_xy", "stride")
AFF_FAULTS = (None, "trunc32", "noclip", "section0", "neighbour_mask", "seam")


@functools.lru_cache(maxsize=None)
def aff_case(roi, name):
    return (_aff_roi if roi else _aff)(name)


def _shift(shape, off):
    dst, src = [], []
    for o, n in zip(off, shape):
        lo, hi = max(0, -o), min(n, n - o)
        dst.append(slice(lo, hi))
        src.append(slice(lo + o, hi + o))
    return tuple(dst), tuple(src)


def _balance(affs, mask, frac):
    with np.errstate(divide="ignore"):
        w_pos, w_neg = np.float32(1.0) / np.float32(2.0 * frac), np.float32(1.0) / np.float32(2.0 * (1.0 - frac))
    return np.where(mask > 0, np.where(affs > 0, w_pos, w_neg), np.float32(0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def aff_reference(roi, name, fault=None):
    """oracle/train_ref.py on every sample on its own (GrowBoundary, AddAffinities, the mask of known voxels), cropped to the
    ROI, BalanceLabels restated on the crop of every sample.  -> dict: grown (the labels' shape), affs / mask / weights
    [n][S][d][h][w] (without [S] for the whole-array entry), frac [S]: a sample's fraction of positives before the clip (None
    without a masked voxel).  `fault`: one of AFF_FAULTS, what a wrong kernel would give instead."""
    from oracle import train_ref as TR
    assert fault in AFF_FAULTS
    c = aff_case(roi, name)
    labels = c.labels if roi else c.labels[None]
    unl = None if c.unl is None else (c.unl if roi else c.unl[None])
    S = labels.shape[0]
    work = labels & 0xFFFFFFFF if fault == "trunc32" else labels
    if fault == "seam":
        assert not c.only_xy and S > 1
        stack = TR.grow_boundary(work.reshape((-1,) + work.shape[2:]), None if unl is None else unl.reshape((-1,) + unl.shape[2:]), c.steps, False)
        grown = stack.reshape(work.shape)
    else:
        grown = np.stack([TR.grow_boundary(work[s], None if unl is None else unl[s], c.steps, c.only_xy) for s in range(S)])
    crop = (slice(None),) + (tuple(slice(o, o + n) for o, n in zip(c.roi_offset, c.roi_shape)) if roi else (slice(None),) * 3)
    affs, masks, fracs, weights = [], [], [], []
    for s in range(S):
        a, m = TR.affinities_from_labels(grown[s], c.nhood)
        if unl is not None:
            if fault == "neighbour_mask":
                for e, off in enumerate(c.nhood):
                    dst, src = _shift(grown[s].shape, off)
                    m[(e,) + dst] *= unl[s][src] > 0
            else:
                m = m * (unl[s] > 0)[None]
        a, m = a[crop], m[crop].astype(np.float32)
        affs.append(a)
        masks.append(m)
        fracs.append(float((a * m).sum()) / float(m.sum()) if m.sum() else None)
    for s in range(S):
        if fault is None:
            weights.append(TR.balance_labels(affs[s], masks[s]))
            continue
        frac = fracs[0 if fault == "section0" else s]
        frac = 0.0 if frac is None else frac
        weights.append(_balance(affs[s], masks[s], frac if fault == "noclip" else min(max(frac, 0.05), 0.95)))
    if fault == "trunc32":   # a 32-bit compare decides wrongly, the labels written are still the 64-bit ones
        grown = np.where(grown != 0, labels, 0)
    out = {"grown": grown, "affs": np.stack(affs, axis=1), "mask": np.stack(masks, axis=1), "weights": np.stack(weights, axis=1), "frac": fracs}
    if not roi:
        out = {k: (v[0] if k == "grown" else v if k == "frac" else v[:, 0]) for k, v in out.items()}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- summed-area table of mask sections -------------------------------------------------------------------------------
SAT_NAMES = ("values", "single", "ones")


@functools.lru_cache(maxsize=None)
def sat_case(name):
    rng = np.random.default_rng(sum(name.encode()) + 4000)
    if name == "values":        # 393 rows and 903 columns of table: more than one workgroup of either; values beyond 0 / 1
        m = rng.choice(np.array([0, 1, 7, 255], np.uint8), size=(3, 130, 300))
        m[1] = 1                # an all-ones section
    elif name == "single":
        m = np.full((1, 1, 1), 255, np.uint8)
    elif name == "ones":
        m = np.ones((2, 37, 53), np.uint8)
    else:
        raise KeyError(name)
    m.setflags(write=False)
    return m


def sat_reference(mask, fault=None):
    """sat[s][y][x] = #{(y', x') : y' < y, x' < x, mask[s][y'][x'] != 0}; fault "sum": the values summed instead"""
    assert fault in (None, "sum")
    s, h, w = mask.shape
    ref = np.zeros((s, h + 1, w + 1), np.int64)
    ref[:, 1:, 1:] = (mask.astype(np.int64) if fault == "sum" else (mask != 0).astype(np.int64)).cumsum(1).cumsum(2)
    return ref
