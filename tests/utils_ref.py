"""Plain numpy / scipy statement of what `bs utils` computes, after the reference's data/mask.py,
data/scale_pyramid.py, data/bbox.py and data/merge.py.  Not a test file: tests/test_utils_cpu.py pins the argument the mask driver
relies on with it, and tests/test_utils_gpu.py holds the kernels of csrc/utils.hip and the drivers bit-equal to it."""
import numpy as np
from scipy import ndimage as ndi

HALO = 21     # data/mask.py:104
RADIUS = 10   # data/mask.py:25


def disk(r):
    """skimage.morphology.disk"""
    c = np.arange(-r, r + 1)
    return (c[:, None] ** 2 + c[None, :] ** 2 <= r * r).astype(np.uint8)


def closing(a, fp):
    """skimage.morphology.binary_closing: the dilation sees 0 outside the array, the erosion 1 (ndi.binary_closing, with 0 for
    both passes, is not it)"""
    return ndi.binary_erosion(ndi.binary_dilation(a, fp), fp, border_value=1)


def closing_plane(section, r=RADIUS):
    """one closing of a 2-D section zero-extended to the plane, restricted to the section"""
    pad = 2 * r
    return closing(np.pad(section != 0, pad), disk(r))[pad:-pad, pad:-pad].astype(np.uint8)


def closing_volume(raw, r=RADIUS):
    return np.stack([closing_plane(s, r) for s in raw])


def mask_blockwise(raw, chunks):
    """data/mask.py `make_raw_mask` over the reference's block grid: write blocks of one chunk from the volume's first voxel (the
    last of an axis shrunk to the volume), read blocks grown by (0, 21, 21) and zero-filled outside the volume, two closings with
    the three-plane footprint, the write block cut out"""
    d = disk(RADIUS)
    fp = np.stack([np.zeros_like(d), d, np.zeros_like(d)])
    padded = np.pad(raw, ((0, 0), (HALO, HALO), (HALO, HALO)))
    out = np.zeros(raw.shape, np.uint8)
    for z in range(0, raw.shape[0], chunks[0]):
        for y in range(0, raw.shape[1], chunks[1]):
            for x in range(0, raw.shape[2], chunks[2]):
                z1, y1, x1 = (min(o + c, n) for o, c, n in zip((z, y, x), chunks, raw.shape))
                block = padded[z:z1, y:y1 + 2 * HALO, x:x1 + 2 * HALO]
                res = closing(closing(block, fp), fp)
                out[z:z1, y:y1, x:x1] = res[:, HALO:HALO + y1 - y, HALO:HALO + x1 - x]
    return out


def _snapped(a, factor, lead, out_shape):
    """the array over the zero-filled ROI of the next level: `lead` voxels in front, up to out_shape * factor behind"""
    back = [o * k - l - n for o, k, l, n in zip(out_shape, factor, lead, a.shape)]
    assert all(b >= 0 for b in back)
    return np.pad(a, list(zip(lead, back)))


def downscale_mean(a, factor, lead, out_shape):
    """skimage.measure.block_reduce(in_data, factor, np.mean) stored into the array's integer dtype"""
    p = _snapped(a, factor, lead, out_shape)
    blocks = p.reshape(out_shape[0], factor[0], out_shape[1], factor[1], out_shape[2], factor[2])
    return blocks.mean(axis=(1, 3, 5)).astype(a.dtype)


def sample_down(a, factor, lead, out_shape):
    """in_data[tuple(slice(k // 2, None, k) for k in factor)]"""
    return _snapped(a, factor, lead, out_shape)[tuple(slice(k // 2, None, k) for k in factor)]


def repeat_up(a, factor):
    for axis, k in enumerate(factor):
        a = np.repeat(a, k, axis=axis)
    return a


def bbox(a, padding=0):
    """data/bbox.py: the slices of the padded, clipped bounding box of a > 0"""
    found = ndi.find_objects(a > 0)[0]
    return tuple(slice(max(0, s.start - padding), min(s.stop + padding, n)) for s, n in zip(found, a.shape))


def merge(a, merges):
    """data/merge.py `quick_merge_block`: a value takes the first key (in file order) whose list holds it"""
    out = a.astype(np.uint64)
    for val in np.unique(a):
        key = next((k for k, ids in merges.items() if int(val) in ids), None)
        if key is not None:
            out[a == val] = np.uint64(int(key))
    return out
