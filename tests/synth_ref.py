"""numpy / scipy restatement of the synthetic-label rules of csrc/synth.hip, for the tests.

Each function states one rule by the shortest route numpy offers, not by the device's route: the dilation shifts whole
sections, the feature transform compares every voxel with every feature, the erosion of grow_boundary is scipy's own.
Volumes are (D, H, W); a raster index is (z * H + y) * W + x."""
import numpy as np
from scipy import ndimage

from bootstrapper_amd.synth_labels import GAUSS_RADIUS, GAUSS_SIGMA, binary_structure, disk, draw_operations, ellipse, grow_steps, star


def dilate_section(sec, struct, iterations):
    """scipy.ndimage.binary_dilation(sec, structure=struct, iterations=iterations): origin at the centre (size // 2),
    zero outside the section: out[y, x] = OR over the set (r, c) of in[y - (r - cy), x - (c - cx)]"""
    sec = np.asarray(sec, dtype=bool)
    struct = np.asarray(struct, dtype=bool)
    h, w = sec.shape
    cy, cx = struct.shape[0] // 2, struct.shape[1] // 2
    for _ in range(int(iterations)):
        out = np.zeros_like(sec)
        for r, c in zip(*np.nonzero(struct)):
            dy, dx = r - cy, c - cx
            ys, yd = slice(max(0, -dy), min(h, h - dy)), slice(max(0, dy), min(h, h + dy))
            xs, xd = slice(max(0, -dx), min(w, w - dx)), slice(max(0, dx), min(w, w + dx))
            out[yd, xd] |= sec[ys, xs]
        sec = out
    return sec


def dilate_points(shape, points, structs, struct_index, iterations):
    vol = np.zeros(shape, dtype=bool)
    for z, y, x in np.asarray(points).reshape(-1, 3):
        vol[z, y, x] = True
    return np.stack([dilate_section(vol[z], structs[int(struct_index[z])], iterations[z]) for z in range(shape[0])]).astype(np.int32)


def label(vol):
    """26-connected components of equal non-zero values; ids = raster ranks of the components' first voxels, from 1
    (skimage.measure.label's default)."""
    vol = np.asarray(vol)
    comp = np.zeros(vol.shape, dtype=np.int64)
    nxt = 0
    for v in np.unique(vol):
        if v == 0:
            continue
        lab, n = ndimage.label(vol == v, structure=np.ones((3, 3, 3), dtype=bool))
        comp[lab > 0] = lab[lab > 0] + nxt
        nxt += n
    flat = comp.ravel()
    ids, first = np.unique(flat, return_index=True)
    ids, first = ids[ids > 0], first[ids > 0]
    lut = np.zeros(nxt + 1, dtype=np.int32)
    lut[ids[np.argsort(first)]] = np.arange(1, len(ids) + 1)
    return lut[comp], len(ids)


def nearest_feature(fg):
    """(d2, index): squared distance to, and raster index of, the nearest True voxel of fg for every voxel; among
    equidistant ones the lowest raster index.  Every voxel against every feature."""
    fg = np.asarray(fg, dtype=bool)
    coords = np.stack(np.nonzero(fg), axis=1).astype(np.int64)      # raster order
    feat = np.flatnonzero(fg.ravel())
    allc = np.stack(np.unravel_index(np.arange(fg.size), fg.shape), axis=1).astype(np.int64)
    d2 = np.empty(fg.size, dtype=np.int64)
    idx = np.empty(fg.size, dtype=np.int64)
    step = max(1, (1 << 24) // max(1, len(coords)))
    for a in range(0, fg.size, step):
        d = ((allc[a:a + step, None, :] - coords[None, :, :]) ** 2).sum(axis=2)
        k = d.argmin(axis=1)                                         # the first minimum: the lowest raster index
        d2[a:a + step] = d[np.arange(len(k)), k]
        idx[a:a + step] = feat[k]
    return d2.reshape(fg.shape), idx.reshape(fg.shape)


def expand(labels, depth, fill):
    labels = np.asarray(labels)
    if not labels.any():
        return np.full(labels.shape, fill, dtype=np.int32)
    d2, idx = nearest_feature(labels != 0)
    return np.where(d2 <= depth * depth, labels.ravel()[idx], fill).astype(np.int32)


def tubes(fg):
    lab, n = label(fg)
    return label(expand(lab, fg.shape[0], n + 1))


def gaussian(noise):
    """scipy's float64 result: gaussian_filter(sigma=10), truncated at 4 sigma, border `reflect`"""
    return ndimage.gaussian_filter(np.asarray(noise, dtype=np.float64), GAUSS_SIGMA, mode="reflect", truncate=GAUSS_RADIUS / GAUSS_SIGMA)


def gaussian_gate(peak=1.0):
    """|float32 device result - float64 result| for inputs of magnitude <= peak: a pass is a sum of n = 2 r + 1 products
    with non-negative weights that sum to 1, so (standard bound of a length-n float32 sum, u = 2^-24) it errs by at most
    (n + 2) u peak -- n for the accumulation, 1 for the weights' rounding to float32, 1 for its input's -- and passes on
    the error of the pass before unamplified; three passes."""
    return 3 * (2 * GAUSS_RADIUS + 1 + 2) * 2.0 ** -24 * peak


def _better(cv, ci, bv, bi):
    return (cv > bv) | ((cv == bv) & (ci < bi))


def argmax_filter(fld, window):
    """raster index of the largest value in the window [-(w // 2), w - 1 - w // 2]^3 with scipy's `reflect` border
    (np.pad's `symmetric`), among equal values the lowest raster index.  Axis by axis: the maximum over a box under a
    total order is the maximum of the maxima of its rows."""
    fld = np.asarray(fld)
    bv = fld.copy()
    bi = np.arange(fld.size, dtype=np.int64).reshape(fld.shape)
    lo, hi = window // 2, window - 1 - window // 2
    for ax in range(3):
        pad = [(0, 0)] * 3
        pad[ax] = (lo, hi)
        pv, pi = np.pad(bv, pad, mode="symmetric"), np.pad(bi, pad, mode="symmetric")
        n = fld.shape[ax]
        nv, ni = None, None
        for t in range(window):
            sl = [slice(None)] * 3
            sl[ax] = slice(t, t + n)
            cv, ci = pv[tuple(sl)], pi[tuple(sl)]
            if nv is None:
                nv, ni = cv.copy(), ci.copy()
            else:
                b = _better(cv, ci, nv, ni)
                nv, ni = np.where(b, cv, nv), np.where(b, ci, ni)
        bv, bi = nv, ni
    return bi.astype(np.int32)


def argmax_filter_brute(fld, window):
    """the same, every window position visited (small volumes and windows)"""
    fld = np.asarray(fld)
    lo, hi = window // 2, window - 1 - window // 2
    pv = np.pad(fld, [(lo, hi)] * 3, mode="symmetric")
    pi = np.pad(np.arange(fld.size, dtype=np.int64).reshape(fld.shape), [(lo, hi)] * 3, mode="symmetric")
    d, h, w = fld.shape
    bv, bi = None, None
    for a in range(window):
        for b in range(window):
            for c in range(window):
                cv, ci = pv[a:a + d, b:b + h, c:c + w], pi[a:a + d, b:b + h, c:c + w]
                if bv is None:
                    bv, bi = cv.copy(), ci.copy()
                else:
                    t = _better(cv, ci, bv, bi)
                    bv, bi = np.where(t, cv, bv), np.where(t, ci, bi)
    return bi.astype(np.int32)


def basins(fld, pos, mask=None):
    """Voxels ordered by (value, lower raster index wins).  parent = the best 6-neighbour if it beats the voxel, else
    pos if that is another voxel (one that beats it), else the voxel itself (a root); label = raster rank of the root."""
    fld = np.asarray(fld)
    d, h, w = fld.shape
    n = fld.size
    m = np.ones(fld.shape, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    idx = np.arange(n, dtype=np.int64).reshape(fld.shape)
    bv, bi = fld.copy(), idx.copy()
    for ax in range(3):
        for sgn in (-1, 1):
            src = [slice(None)] * 3
            dst = [slice(None)] * 3
            src[ax] = slice(1, None) if sgn > 0 else slice(None, -1)
            dst[ax] = slice(None, -1) if sgn > 0 else slice(1, None)
            src, dst = tuple(src), tuple(dst)
            b = m[src] & _better(fld[src], idx[src], bv[dst], bi[dst])
            bv[dst], bi[dst] = np.where(b, fld[src], bv[dst]), np.where(b, idx[src], bi[dst])
    par = bi.ravel().copy()
    own = par == np.arange(n)
    p = np.asarray(pos).ravel().astype(np.int64)
    ok = own & (p >= 0) & (p < n)
    pc = np.clip(p, 0, n - 1)
    ok &= m.ravel()[pc] & _better(fld.ravel()[pc], pc, fld.ravel(), np.arange(n))
    par[ok] = p[ok]
    par[~m.ravel()] = -1
    root = par.copy()
    while True:
        nxt = np.where(root >= 0, root[np.maximum(root, 0)], -1)
        if np.array_equal(nxt, root):
            break
        root = nxt
    roots = np.flatnonzero(par == np.arange(n))
    rank = np.zeros(n + 1, dtype=np.int32)
    rank[roots] = np.arange(1, len(roots) + 1)
    return np.where(root >= 0, rank[np.maximum(root, 0)], 0).reshape(fld.shape).astype(np.int32), len(roots)


def finish(labels, drop3, drop5, anisotropy):
    labels = np.asarray(labels).copy()
    for flag, div in ((drop3, 3), (drop5, 5)):
        if flag:
            labels[labels % div == 0] = 0
    out = labels[::anisotropy] if anisotropy <= labels.shape[0] else labels[0:1]
    return out.astype(np.int64)


def grow_boundary(labels, seed, max_steps):
    """custom_grow_boundary.py with only_xy=True and no mask; the step count of (section, label) is the counter hash"""
    gt = np.asarray(labels).copy()
    for z in range(gt.shape[0]):
        fg = np.zeros(gt[z].shape, dtype=bool)
        for lab in np.unique(gt[z]):
            if lab == 0:
                continue
            m = gt[z] == lab
            steps = grow_steps(seed, z, int(lab), max_steps)
            fg |= ndimage.binary_erosion(m, iterations=steps, border_value=1) if steps > 0 else m
        gt[z][~fg] = 0
    return gt


def merge(labels, sections, a, b):
    out = np.asarray(labels).copy()
    for z in sections:
        out[z][out[z] == b] = a
    return out


def stamp(labels, z, y, x, struct, value):
    out = np.asarray(labels).copy()
    s = np.asarray(struct, dtype=bool)
    view = out[z, y:y + s.shape[0], x:x + s.shape[1]]
    view[s] = value
    return out


def split_field(mask):
    """squared Euclidean distance to the nearest voxel outside the mask, 0 outside it; the volume's border is no
    background (edt.edt's black_border=False, scipy's behaviour); 2^30 where the mask is the whole volume"""
    mask = np.asarray(mask, dtype=bool)
    if mask.all():
        return np.full(mask.shape, 2.0 ** 30, dtype=np.float32)
    return np.rint(ndimage.distance_transform_edt(mask) ** 2).astype(np.float32)


def split(labels, label_id, window, sections, scale):
    """obfuscate_labels.py:88-104 by the specified rule -> (labels, number of fragments)"""
    out = np.asarray(labels).copy()
    mask = out == label_id
    fld = split_field(mask)
    frag, n = basins(fld, argmax_filter(fld, window), mask)
    for z in sections:
        out[z] = np.where(mask[z], frag[z].astype(np.int64) * scale, out[z])
    return out, n


def obfuscate(labels, rng, num_tries=5, p_split=0.1, p_merge=0.1, p_artifact=0.1):
    """obfuscate_labels.py:50-143 with `rng` for the random module: the same draws in the same order"""
    labels = np.asarray(labels).copy()
    unique = [int(v) for v in np.unique(labels) if v != 0]
    if not unique:
        return labels
    d, h, w = labels.shape
    for op in draw_operations(rng, num_tries, p_split, p_merge, p_artifact):
        if op == "split" and len(unique) > 0:
            label_id = rng.choice(unique)
            window = rng.randint(15, 50)
            zs = rng.sample(range(d), k=rng.randint(1, 2))
            labels = split(labels, label_id, window, zs, int(labels.max()))[0]
            unique = [int(v) for v in np.unique(labels[labels != 0])]
        if op == "merge" and len(unique) >= 2:
            zs = rng.sample(range(d), k=rng.randint(1, 2))
            a, b = rng.sample(list(unique), 2)
            labels = merge(labels, zs, a, b)
            unique = [v for v in unique if v != b]
        if op == "artifact" and len(unique) > 0:
            structs = [star(rng.randint(2, 8)), binary_structure(rng.randint(1, 2)), disk(rng.randint(1, 8)), ellipse(rng.randint(2, 8), rng.randint(2, 8))]
            new_label = int(labels.max()) + 1
            for z in rng.sample(range(d), k=rng.randint(1, 2)):
                art = rng.choice(structs)
                y, x = rng.randint(0, h - art.shape[0]), rng.randint(0, w - art.shape[1])
                labels = stamp(labels, z, y, x, art, new_label)
                new_label += 1
    return labels
