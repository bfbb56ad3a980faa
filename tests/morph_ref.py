"""Plain numpy statement of the rule behind `bs refine morph` (include/bsmi.h): label-preserving dilate /
erode / opening / closing / fill_holes on the array A that one operation sees (a 2-D section or a 3-D block), and the
reference's per-block driver (refine.py:47-72, 347-360) on top of `bootstrapper_amd.refine.morph_blocks`.  fastmorph, which the
reference calls, is not installed: the rule is this project's own and tests/test_morph_pin.py reports its parity as unpinned.
The kernels of csrc/morph.hip are held bit-equal to this file by tests/test_morph_gpu.py."""
import itertools

import numpy as np
from scipy import ndimage

MERGE_THRESHOLD = (19, 20)   # 20 n_L >= 19 T


def _stencil(a):
    """(3^ndim, *a.shape): every stencil position's value per voxel, 0 outside the array, centre in the middle"""
    pad = np.pad(a, 1)
    offs = list(itertools.product((0, 1, 2), repeat=a.ndim))
    return np.stack([pad[tuple(slice(o, o + n) for o, n in zip(off, a.shape))] for off in offs])


def neighbour_counts(a):
    """for the background voxels with a labelled stencil neighbour: (their flat indices, stencil values S [N][M], counts C [N][M]
    with C[i] = how often S[i] occurs in the voxel's stencil, 0 where S[i] == 0)"""
    s = _stencil(a).reshape(3 ** a.ndim, -1)
    at = np.nonzero((a.ravel() == 0) & (s != 0).any(0))[0]
    s = s[:, at]
    c = np.zeros(s.shape, np.int64)
    for i in range(s.shape[0]):
        c[i] = (s == s[i]).sum(0)
    c[s == 0] = 0
    return at, s, c


def tied_voxels(a):
    """number of background voxels whose most frequent neighbouring id is shared by two or more ids"""
    _, s, c = neighbour_counts(a)
    top = c == c.max(0)
    lo = np.where(top, s, np.iinfo(np.uint64).max).min(0)
    hi = np.where(top, s, 0).max(0)
    return int((lo != hi).sum())


def dilate_step(a):
    at, s, c = neighbour_counts(a)
    out = a.copy()
    if at.size:
        top = c == c.max(0)
        out.ravel()[at] = np.where(top, s, np.iinfo(a.dtype).max).min(0)   # ties: the smallest id
    return out


def erode_step(a):
    return np.where((_stencil(a) == a).all(0), a, 0).astype(a.dtype)


def fill_holes(a):
    face = ndimage.generate_binary_structure(a.ndim, 1)
    out = a.copy()
    for i in np.unique(a):
        lab, n = ndimage.label(a == i, structure=face)
        for k, box in enumerate(ndimage.find_objects(lab), 1):
            if any(s.start == 0 or s.stop == m for s, m in zip(box, a.shape)):
                continue   # a voxel on a face of A
            grown = tuple(slice(s.start - 1, s.stop + 1) for s in box)
            inside = lab[grown] == k
            ids = a[grown]
            faces = {}
            for axis in range(a.ndim):
                for shift in (1, -1):
                    nb_in = np.roll(inside, shift, axis)   # the box is grown by one: nothing of C wraps round
                    nb_id = np.roll(ids, shift, axis)
                    for v in nb_id[inside & ~nb_in]:
                        faces[int(v)] = faces.get(int(v), 0) + 1
            total = sum(faces.values())
            best = max(((cnt, -v) for v, cnt in faces.items() if v != 0), default=None)
            if best is not None and MERGE_THRESHOLD[1] * best[0] >= MERGE_THRESHOLD[0] * total:
                out[grown][inside] = -best[1]
    return out


def apply_array(a, op, iterations=1):
    """one operation on the array A = a (2-D or 3-D)"""
    def times(step, x):
        for _ in range(iterations):
            x = step(x)
        return x
    if op == "dilate":
        return times(dilate_step, a)
    if op == "erode":
        return times(erode_step, a)
    if op == "opening":
        return times(dilate_step, times(erode_step, a))
    if op == "closing":
        return times(erode_step, times(dilate_step, a))
    if op == "fill_holes":
        return fill_holes(a)
    raise ValueError(op)


def apply_block(block, op, iterations=1, xy=False):
    """what the reference's `_morph_block` computes on a read block (refine.py:351-356)"""
    if not xy:
        return apply_array(block, op, iterations)
    return np.stack([apply_array(block[z], op, iterations) for z in range(block.shape[0])])


def morph_volume(vol, chunks, op, iterations=1, xy=False, context=64, block_size=2048):
    """the blockwise result: every read block on its own, its write block cut out"""
    from bootstrapper_amd.refine import morph_blocks
    out = np.zeros_like(vol)
    for write, read in morph_blocks(vol.shape, chunks, block_size, context, xy):
        res = apply_block(vol[tuple(slice(lo, hi) for lo, hi in read)], op, iterations, xy)
        out[tuple(slice(lo, hi) for lo, hi in write)] = res[tuple(slice(w[0] - r[0], w[1] - r[0]) for w, r in zip(write, read))]
    return out


def cells(shape, n, seed, gap=0.55, big_ids=True, voids=5):
    """seeded test labels: Voronoi cells (touching labels) with thin background gaps along some cell borders, a few
    background specks and `voids` wider background boxes (several dilations deep); ids are spread up to above 2^32 when
    big_ids"""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.integers(0, s, n) for s in shape], 1)
    ids = rng.permutation(np.arange(1, n + 1)).astype(np.uint64)
    if big_ids:
        ids[::3] += np.uint64(1 << 33)
        ids[1::5] = np.uint64((1 << 64) - 1) - ids[1::5]
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3)
    d = np.sqrt(((grid[:, None, :] - pts[None, :, :]) ** 2).sum(-1).astype(np.float64))
    order = np.argsort(d, 1)[:, :2]
    near, second = np.take_along_axis(d, order, 1).T
    out = ids[order[:, 0]]
    cut = (second - near < gap) & (rng.random(near.size) < 0.7)
    out[cut] = 0
    out[rng.random(near.size) < 0.01] = 0
    out = out.reshape(shape)
    for _ in range(voids):
        lo = [int(rng.integers(0, s)) for s in shape]
        out[tuple(slice(o, o + int(rng.integers(4, 15))) for o in lo)] = 0
    return out


def contact_case(foreign):
    """a background hole of 1 x 1 x 25 voxels inside label 5: 102 faces, `foreign` of them against label 6 (6 -> 96 / 102 =
    94.1 % of the faces against 5, 5 -> 97 / 102 = 95.1 %)"""
    a = np.full((5, 5, 31), 5, np.uint64)
    a[2, 2, 3:28] = 0
    for k in range(foreign):
        a[1, 2, 3 + 2 * k] = 6   # isolated voxels of 6 above the hole, each one face of it
    return a


def holes(shape, seed, n=12):
    """`cells` without gaps, with enclosed cavities, foreign specks, cavities cut by the array's faces and nested ones added"""
    rng = np.random.default_rng(seed)
    a = cells(shape, n, seed, gap=0.0, voids=0)
    for _ in range(60):
        lo = [int(rng.integers(0, s)) for s in shape]
        ext = [int(rng.integers(1, 4)) for _ in shape]
        box = tuple(slice(o, o + e) for o, e in zip(lo, ext))
        a[box] = 0 if rng.random() < 0.6 else np.uint64(rng.integers(100, 104))
    return a
