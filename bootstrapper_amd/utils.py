"""`bs utils` on the device: mask, scale_pyramid, bbox and merge.

Same commands, options, defaults and default output names as the reference's `utils.py` (`data/mask.py`,
`data/scale_pyramid.py`, `data/bbox.py`, `data/merge.py`); `convert` (image file readers, no device work) and `download_ckpts`
(network) are not built.  The kernels are csrc/utils.hip (include/bsmi.h "volume utilities"); the rules, the argument why the raw
mask does not depend on the block grid, the declared differences and what is refused are DESIGN.md section 7h, restated in
tests/utils_ref.py.
"""
import collections
import ctypes as C
import json
import os
import re

import click
import numpy as np

from .zarr_io import open_ds, prepare_ds

MASK_RADIUS = 10        # disk(10), data/mask.py:25
WRITES_IN_FLIGHT = 2    # tiles queued for writing before the next one waits
LABEL_WORDS = ("label", "lbl", "ids", "mask", "seg")   # data/scale_pyramid.py:16
_INT_VIEW = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}


# ---- device calls ----

def _stream(t):
    import torch
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _i32x3(v):
    return (C.c_int32 * 3)(*[int(x) for x in v])


def _upload(a, dev):
    """a numpy integer array as a CUDA tensor of the signed type of its width (torch has no arithmetic on the wide unsigned ones)"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_INT_VIEW[a.dtype.itemsize])).to(dev)


def _download(t, dtype):
    return t.cpu().numpy().view(dtype)


def _free_bytes(dev):
    """what the driver reports plus what this process's allocator holds without using it"""
    import torch
    return torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)


def closing_work_bytes(shape, radius):
    from . import _lib
    return int(_lib.lib.bsmi_mask_closing_work_bytes(_lib.i64x3(shape), int(radius)))


def mask_closing(raw, radius=MASK_RADIUS, out=None, work=None):
    """bsmi_mask_closing_disk_u8 on a contiguous uint8 CUDA tensor [D][H][W]: every section closed by the disk of `radius`, as the
    section zero-extended to the plane -> uint8 0 / 1.  Asynchronous on the current stream."""
    import torch
    from . import _lib
    if raw.dtype not in (torch.uint8, torch.int8) or not raw.is_cuda or raw.dim() != 3 or not raw.is_contiguous():
        raise ValueError("raw must be a contiguous 8-bit CUDA tensor of shape (D, H, W)")
    out = torch.empty(raw.shape, dtype=torch.uint8, device=raw.device) if out is None else out
    need = closing_work_bytes(raw.shape, radius)
    if work is None:
        work = torch.empty(max(1, (need + 7) // 8), dtype=torch.int64, device=raw.device)
    _lib.check(_lib.lib.bsmi_mask_closing_disk_u8(raw.device.index, _ptr(raw), _lib.i64x3(raw.shape), int(radius), _ptr(out), _ptr(work),
                                                  work.numel() * work.element_size(), _stream(raw)))
    return out


def rescale(vol, factor, lead, out_shape, how):
    """one level of a pyramid on a contiguous integer CUDA tensor [D][H][W]; how: "mean" (8 / 16 bit), "down" (sample) or "up"
    (repeat).  include/bsmi.h bsmi_downscale_mean / bsmi_rescale_sample.  Asynchronous on the current stream."""
    import torch
    from . import _lib
    if not vol.is_cuda or vol.dim() != 3 or not vol.is_contiguous():
        raise ValueError("vol must be a contiguous CUDA tensor of shape (D, H, W)")
    out = torch.empty(tuple(int(s) for s in out_shape), dtype=vol.dtype, device=vol.device)
    args = (vol.device.index, _ptr(vol), vol.element_size(), _lib.i64x3(vol.shape), _i32x3(factor), _i32x3(lead))
    if how == "mean":
        _lib.check(_lib.lib.bsmi_downscale_mean(*args, _ptr(out), _lib.i64x3(out_shape), _stream(vol)))
    else:
        mode = {"down": _lib.RESCALE_DOWN, "up": _lib.RESCALE_UP}[how]
        _lib.check(_lib.lib.bsmi_rescale_sample(*args, mode, _ptr(out), _lib.i64x3(out_shape), _stream(vol)))
    return out


def new_box(dev):
    import torch
    big = np.iinfo(np.int64).max
    return torch.tensor([big, big, big, -1, -1, -1], dtype=torch.int64, device=dev)


def nonzero_bbox(vol, origin, box):
    """merge the extremes of (z, y, x) + origin over the non-zero voxels of `vol` into `box` (new_box); asynchronous"""
    from . import _lib
    if not vol.is_cuda or vol.dim() != 3 or not vol.is_contiguous():
        raise ValueError("vol must be a contiguous CUDA tensor of shape (D, H, W)")
    _lib.check(_lib.lib.bsmi_nonzero_bbox(vol.device.index, _ptr(vol), vol.element_size(), _lib.i64x3(vol.shape), _lib.i64x3(origin), _ptr(box),
                                          _stream(vol)))
    return box


class _WriteBehind:
    """dataset writes on one host thread, at most WRITES_IN_FLIGHT of them queued"""

    def __init__(self):
        from concurrent.futures import ThreadPoolExecutor
        self.pool = ThreadPoolExecutor(1)
        self.queued = collections.deque()

    def submit(self, ds, key, data):
        while len(self.queued) >= WRITES_IN_FLIGHT:
            self.queued.popleft().result()
        self.queued.append(self.pool.submit(ds.__setitem__, key, data))

    def close(self, wait=True):
        try:
            while wait and self.queued:
                self.queued.popleft().result()
        finally:
            self.pool.shutdown(wait=True)


# ---- mask ----

def _split_zarr(path, what):
    parts = path.split(".zarr")
    if len(parts) != 2:
        raise click.ClickException(f"no default output name for {path!r}: give {what}")
    return parts


def mask_tiles(shape, chunks, tile, halo):
    """(write, read) boxes of the raw-mask driver: one chunk along z, `tile` = (rows, columns) snapped to whole chunks along y and
    x; the read box is the write box grown by `halo` in y and x and clipped to the volume (outside it the kernel sees 0 anyway)"""
    cz, cy, cx = (int(c) for c in chunks)
    step = (cz, cy * max(1, tile[0] // cy), cx * max(1, tile[1] // cx))
    out = []
    for z in range(0, shape[0], step[0]):
        for y in range(0, shape[1], step[1]):
            for x in range(0, shape[2], step[2]):
                write = tuple((o, min(o + s, int(n))) for o, s, n in zip((z, y, x), step, shape))
                read = (write[0],) + tuple((max(0, lo - halo), min(int(n), hi + halo)) for (lo, hi), n in zip(write[1:], shape[1:]))
                out.append((write, read))
    return out


def _default_mask_tile(shape, chunks):
    """whole rows of x, and as many rows as keep a tile (one chunk of sections) near 2^28 voxels"""
    cz = min(int(chunks[0]), int(shape[0]))
    rows = max(1, (1 << 28) // max(1, cz * int(shape[2])))
    return (max(rows, int(chunks[1])), int(shape[2]))


def mask(in_array, out_array=None, mode=None, device=0, tile=None):
    """Generate a mask of a zarr image ("raw") or labels ("labels") array (data/mask.py:84-143).

    labels: in > 0.  raw: the closing of every z section by disk(10); one closing of a tile with a halo of 20 equals the
    reference's two closings per chunk-shaped block with a halo of 21.  `tile` = (rows, columns) of a
    tile of the raw mode, snapped to whole chunks (default: whole rows of x, about 2^28 voxels)."""
    import torch
    if mode not in ("raw", "labels"):
        raise click.ClickException("--mode must be raw or labels")
    in_ds = open_ds(in_array)
    if in_ds.dtype.kind not in "iu":
        raise click.ClickException(f"{in_array}: mask takes an integer dataset, not {in_ds.dtype}")
    if mode == "raw" and (len(in_ds.shape) != 3 or in_ds.dtype.itemsize != 1):
        raise click.ClickException(f"{in_array}: the raw mask takes a 3-D 8-bit dataset, not {in_ds.shape} {in_ds.dtype}")
    if out_array is None:
        in_f, name = _split_zarr(in_array, "--out_array")
        out_array = f"{in_f}.zarr/{name.strip('/').replace(mode, f'{mode}_mask')}"
    print(f"Writing mask to {out_array}")
    dev = torch.device("cuda", device)
    keep = dict(shape=in_ds.shape, offset=in_ds.offset, voxel_size=in_ds.voxel_size, axis_names=in_ds.axis_names, units=in_ds.units,
                dtype=np.uint8, chunk_shape=in_ds.chunks)
    if mode == "labels":
        out_ds = prepare_ds(out_array, **keep)
        step = int(in_ds.chunks[0])
        writer = _WriteBehind()
        done = False
        try:
            for lo in range(0, in_ds.shape[0], step):
                sl = slice(lo, min(lo + step, in_ds.shape[0]))
                t = _upload(in_ds[sl], dev)
                hit = t > 0 if in_ds.dtype.kind == "i" else t != 0
                writer.submit(out_ds, sl, hit.to(torch.uint8).cpu().numpy())
            done = True
        finally:
            writer.close(done)
        return out_array
    halo = 2 * MASK_RADIUS
    tiles = mask_tiles(in_ds.shape, in_ds.chunks, tile or _default_mask_tile(in_ds.shape, in_ds.chunks), halo)
    extent = lambda box: tuple(hi - lo for lo, hi in box)  # noqa: E731
    most = max((extent(r) for _, r in tiles), key=lambda e: int(np.prod(e)), default=(0, 0, 0))
    # the read tile, its result, the packed dilation
    need = 2 * int(np.prod(most)) + closing_work_bytes(most, MASK_RADIUS)
    free = _free_bytes(dev)
    if need > free:
        raise click.ClickException(f"a tile of {most} voxels with its buffers needs {need / 2**30:.2f} GiB of device memory, "
                                   f"{free / 2**30:.2f} GiB are free: use smaller tiles")
    out_ds = prepare_ds(out_array, **keep)
    writer = _WriteBehind()
    done = False
    try:
        with torch.cuda.device(dev):
            for write, read in tiles:
                raw = torch.from_numpy(np.ascontiguousarray(in_ds[tuple(slice(lo, hi) for lo, hi in read)]).view(np.uint8)).to(dev)
                res = mask_closing(raw)
                cut = res[tuple(slice(w[0] - r[0], w[1] - r[0]) for w, r in zip(write, read))]
                writer.submit(out_ds, tuple(slice(lo, hi) for lo, hi in write), cut.cpu().numpy())
        done = True
    finally:
        writer.close(done)
    return out_array


# ---- scale pyramid ----

def is_label_array(name, dtype):
    """True when the array holds object ids, which must never be averaged: by dtype (u32, u64) or by a word of its name, so that
    a uint8 mask is still safe (data/scale_pyramid.py:19-28)"""
    lowered = os.path.basename(name).lower()
    return np.dtype(dtype) in (np.dtype(np.uint32), np.dtype(np.uint64)) or any(w in lowered for w in LABEL_WORDS)


def parse_factor(value):
    """Comma or space separated integers, as a tuple."""
    return tuple(int(v) for v in value.replace(",", " ").split())


def pyramid_plan(in_array, shape, offset, voxel_size, scales, mode):
    """What `scale_pyramid` will do to the array at `in_array` (spatial `shape`, `offset` and `voxel_size` in world units), as
    data: no file is touched (data/scale_pyramid.py:145-242).
    -> dict(name: the pyramid's name, base: the group's path, renames: [(from, to)] paths in order, start: path of the level the
    input becomes, levels: [dict(name, path, factor, voxel_size, offset, shape, lead)] in the order they are made)."""
    in_array = os.path.normpath(in_array)
    parent, ds_name = os.path.split(in_array)
    dims = len(voxel_size)
    for s in scales:
        if len(s) != dims or any(k < 1 for k in s):
            raise click.ClickException(f"Scale factor {tuple(s)} has {len(s)} values, but {in_array} has {dims} spatial dimensions "
                                       "(every value at least 1).")
    at_level = re.match(r"^s(\d+)$", ds_name)
    renames = []
    if at_level:
        start, base, name = int(at_level.group(1)), parent, os.path.basename(parent)
        if mode == "up" and start - len(scales) < 0:   # no room below: the input becomes the new top
            start = len(scales)
            renames.append((in_array, os.path.join(base, f"s{start}")))
    else:
        start, base, name = (0 if mode == "down" else len(scales)), in_array, ds_name
        renames += [(in_array, in_array + "__tmp"), (in_array + "__tmp", os.path.join(base, f"s{start}"))]
    levels = []
    shape, offset, voxel = [int(v) for v in shape], [int(v) for v in offset], [int(v) for v in voxel_size]
    for i, k in enumerate(scales, 1):
        if mode == "up":
            if any(v % f for v, f in zip(voxel, k)):
                raise click.ClickException(f"voxel size {tuple(voxel)} is not divisible by the scale factor {tuple(k)}")
            nvoxel = [v // f for v, f in zip(voxel, k)]
        else:
            nvoxel = [v * f for v, f in zip(voxel, k)]
        # the ROI snapped outwards to the next voxel grid
        begin = [o // nv * nv for o, nv in zip(offset, nvoxel)]
        end = [-(-(o + n * v) // nv) * nv for o, n, v, nv in zip(offset, shape, voxel, nvoxel)]
        if any((o - b) % v for o, b, v in zip(offset, begin, voxel)):
            raise click.ClickException(f"offset {tuple(offset)} does not lie on the voxel grid {tuple(voxel)} of the level before s{start + (i if mode == 'down' else -i)}")
        lead = [(o - b) // v for o, b, v in zip(offset, begin, voxel)]
        shape, offset, voxel = [(e - b) // nv for e, b, nv in zip(end, begin, nvoxel)], begin, nvoxel
        num = start + (i if mode == "down" else -i)
        levels.append(dict(name=f"s{num}", path=os.path.join(base, f"s{num}"), factor=tuple(int(f) for f in k), voxel_size=tuple(voxel),
                           offset=tuple(offset), shape=tuple(shape), lead=tuple(lead)))
    return dict(name=name, base=base, renames=renames, start=os.path.join(base, f"s{start}"), levels=levels)


def _scale_level(prev, nxt, level, how, dev):
    """one level, every channel, in slabs of one chunk of sections (of the coarser of the two arrays)"""
    import torch
    nd = len(level["factor"])
    pad = 3 - nd   # a 2-D array is one section
    k = (1,) * pad + tuple(level["factor"])
    lead = (0,) * pad + tuple(level["lead"])
    in_sp = (1,) * pad + tuple(prev.shape[-nd:])
    out_sp = (1,) * pad + tuple(level["shape"])
    channels = tuple(prev.shape[:-nd])
    cz = max(1, int(nxt.chunks[-nd])) if nd == 3 else 1
    slabs = []   # (input z range, lead along z, output z range)
    if how == "up":
        step = max(1, int(prev.chunks[-nd])) if nd == 3 else 1
        for lo in range(0, in_sp[0], step):
            hi = min(lo + step, in_sp[0])
            slabs.append(((lo, hi), 0, (lo * k[0], hi * k[0])))
    else:
        for lo in range(0, out_sp[0], cz):
            hi = min(lo + cz, out_sp[0])
            first = lo * k[0] - lead[0]
            slabs.append(((max(0, first), min(in_sp[0], hi * k[0] - lead[0])), max(0, -first), (lo, hi)))
    item = prev.dtype.itemsize
    most = max(((i1 - i0) * in_sp[1] * in_sp[2] + (o1 - o0) * out_sp[1] * out_sp[2] for (i0, i1), _, (o0, o1) in slabs), default=0) * item
    free = _free_bytes(dev)
    if most > free:
        raise click.ClickException(f"a slab of {level['name']} needs {most / 2**30:.2f} GiB of device memory, {free / 2**30:.2f} GiB are free: "
                                   "give a smaller --chunk_shape along z")
    writer = _WriteBehind()
    done = False
    try:
        with torch.cuda.device(dev):
            for c in np.ndindex(*channels):
                for (i0, i1), lz, (o0, o1) in slabs:
                    if i1 <= i0:   # a slab wholly in front of or behind the data: zero fill
                        data = np.zeros((o1 - o0,) + out_sp[1:], prev.dtype)
                    else:
                        src = prev[c + ((slice(i0, i1),) if nd == 3 else ())]
                        vol = _upload(src.reshape((i1 - i0,) + in_sp[1:]), dev)
                        res = rescale(vol, k, (lz,) + lead[1:], (o1 - o0,) + out_sp[1:], how)
                        data = _download(res, prev.dtype)
                    key = c + ((slice(o0, o1),) if nd == 3 else ())
                    writer.submit(nxt, key, data.reshape(data.shape[pad:]))
        done = True
    finally:
        writer.close(done)


def scale_pyramid(in_array, scales, chunk_shape=None, mode=None, device=0):
    """Create a scale pyramid of a zarr array, in place (data/scale_pyramid.py:132-244).

    The array becomes s0 of a group of its own name, and every further level is coarser: s0 is always the finest.  Upscaling
    counts down to s0 instead.  Images (u8, u16) are averaged, label arrays (`is_label_array`) sampled; upscaling an image and
    float images are refused before anything is renamed or written."""
    import torch
    if mode not in ("up", "down"):
        raise click.ClickException("--mode must be up or down")
    in_array = os.path.normpath(in_array)
    prev = open_ds(in_array)
    dims = len(prev.voxel_size)
    scales = [parse_factor(s) if isinstance(s, str) else tuple(int(v) for v in s) for s in scales]
    if not scales:
        raise click.ClickException("give at least one --scales")
    plan = pyramid_plan(in_array, prev.shape[-dims:], prev.offset, prev.voxel_size, scales, mode)
    if chunk_shape is not None:
        chunk = parse_factor(chunk_shape) if isinstance(chunk_shape, str) else tuple(int(v) for v in chunk_shape)
        if len(chunk) != dims:
            raise click.ClickException(f"Chunk shape {chunk} has {len(chunk)} values, but {in_array} has {dims} spatial dimensions.")
    else:
        chunk = tuple(prev.chunks[-dims:])
    labels = is_label_array(plan["name"], prev.dtype)
    print(f"{mode.capitalize()}scaling {in_array} by {scales} ({'labels: sampling' if labels else 'image: averaging'})")
    if dims not in (2, 3):
        raise NotImplementedError(f"{dims} spatial dimensions: scale_pyramid takes 2 or 3")
    if prev.dtype.kind not in "iu":
        raise NotImplementedError(f"{prev.dtype} arrays: scale_pyramid takes integer images (u8, u16) and integer labels")
    if not labels and mode == "up":
        raise NotImplementedError("upscaling an image (skimage rescale, order 1) is not built: only label arrays are upscaled")
    if not labels and (prev.dtype.kind != "u" or prev.dtype.itemsize > 2):
        raise NotImplementedError(f"{prev.dtype} images: averaging is built for uint8 and uint16")
    if not labels and any(int(np.prod(k)) > 65536 for k in scales):
        raise click.ClickException("a window of more than 65536 voxels")
    taken = [p for p in [dst for _, dst in plan["renames"][-1:]] + [lv["path"] for lv in plan["levels"]] if os.path.exists(p)]
    if taken:
        raise click.ClickException(f"{taken[0]} already exists. Remove it or pick another input.")
    for src, dst in plan["renames"]:
        if dst == plan["start"] and src.endswith("__tmp"):   # the group of the array's own name
            os.makedirs(plan["base"])
            with open(os.path.join(plan["base"], ".zgroup"), "w") as f:
                json.dump({"zarr_format": 2}, f)
        print(f"Renaming {src} to {dst}")
        os.rename(src, dst)
    prev = open_ds(plan["start"])
    channels = tuple(prev.shape[:-dims])
    how = ("down" if mode == "down" else "up") if labels else "mean"
    dev = torch.device("cuda", device)
    for level in plan["levels"]:
        print(f"Preparing {level['name']}: voxel size {level['voxel_size']}, offset {level['offset']}, shape {level['shape']}")
        nxt = prepare_ds(level["path"], shape=channels + level["shape"], offset=level["offset"], voxel_size=level["voxel_size"],
                         axis_names=prev.axis_names, units=prev.units, dtype=prev.dtype, chunk_shape=channels + chunk)
        _scale_level(prev, nxt, level, how, dev)
        prev = nxt
    return plan["base"]


# ---- bbox ----

def bbox(in_array, out_array=None, padding=0, device=0):
    """Crop an array to the bounding box of its voxels > 0, grown by `padding` and clipped to the array (data/bbox.py:24-80)."""
    import torch
    in_ds = open_ds(in_array)
    if len(in_ds.shape) != 3 or in_ds.dtype.kind != "u":
        raise click.ClickException(f"{in_array}: bbox takes a 3-D dataset of unsigned integers, not {in_ds.shape} {in_ds.dtype}")
    dev = torch.device("cuda", device)
    step = int(in_ds.chunks[0])
    need = 2 * step * in_ds.shape[1] * in_ds.shape[2] * in_ds.dtype.itemsize
    if need > _free_bytes(dev):
        raise click.ClickException(f"a slab of {step} sections needs {need / 2**30:.2f} GiB of device memory")
    with torch.cuda.device(dev):
        box = new_box(dev)
        for lo in range(0, in_ds.shape[0], step):
            nonzero_bbox(_upload(in_ds[lo:min(lo + step, in_ds.shape[0])], dev), (lo, 0, 0), box)
        box = [int(v) for v in box.cpu().numpy()]
    if box[3] < 0:
        raise click.ClickException(f"{in_array} holds no voxel above 0: there is no bounding box")
    slices = tuple(slice(max(0, box[d] - padding), min(box[3 + d] + 1 + padding, in_ds.shape[d])) for d in range(3))
    new_offset = [in_ds.offset[d] + slices[d].start * in_ds.voxel_size[d] for d in range(3)]
    if out_array is None:
        out_array = os.path.join(os.path.dirname(in_array), os.path.basename(in_array) + "_bbox")
    print(f"Writing to {out_array}")
    shape = tuple(s.stop - s.start for s in slices)
    out_ds = prepare_ds(out_array, shape=shape, offset=new_offset, voxel_size=in_ds.voxel_size, axis_names=in_ds.axis_names, units=in_ds.units,
                        dtype=in_ds.dtype, chunk_shape=in_ds.chunks, mode="w")
    for lo in range(0, shape[0], step):
        hi = min(lo + step, shape[0])
        out_ds[lo:hi] = in_ds[(slice(slices[0].start + lo, slices[0].start + hi),) + slices[1:]]
    return out_array


# ---- merge ----

def merge_mapping(luts):
    """{"merges": {id: [ids]}} -> (keys, values) uint64: a value takes the first key in file order whose list holds it
    (data/merge.py:22-27); keys arrive as strings"""
    table = {}
    for key, ids in luts["merges"].items():
        for v in ids:
            table.setdefault(int(v), int(key))
    keys = np.fromiter(table, dtype=np.uint64, count=len(table))
    return keys, np.array([table[int(k)] for k in keys], dtype=np.uint64)


def merge(in_seg, out_seg=None, luts=None, device=0):
    """Perform the merges of a LUTs file on a segmentation (data/merge.py:60-128); the output is uint64."""
    from .post.engine import lut_relabel
    from .refine import _Device, _apply_mapping, _tiles
    in_ds = open_ds(in_seg)
    if len(in_ds.shape) != 3 or in_ds.dtype.kind != "u":
        raise click.ClickException(f"{in_seg}: merge takes a 3-D dataset of unsigned integer labels, not {in_ds.shape} {in_ds.dtype}")
    with open(luts) as f:
        keys, vals = merge_mapping(json.load(f))
    if out_seg is None:
        in_f, name = _split_zarr(in_seg, "--out_seg")
        out_seg = f"{in_f}.zarr/{name.strip('/')}__merged.zarr"
    print(f"Writing to {out_seg}")
    if in_ds.dtype == np.uint64:
        _apply_mapping(in_ds, out_seg, keys, vals, device)
        return out_seg
    d = _Device(in_ds, device)
    out_ds = prepare_ds(out_seg, shape=in_ds.shape, offset=in_ds.offset, voxel_size=in_ds.voxel_size, axis_names=in_ds.axis_names,
                        units=in_ds.units, dtype=np.uint64, chunk_shape=in_ds.chunks)
    order = np.argsort(keys, kind="stable")
    k = d.torch.from_numpy(keys[order].view(np.int64)).to(d.dev)
    v = d.torch.from_numpy(vals[order].view(np.int64)).to(d.dev)
    for _, sl in _tiles(in_ds):
        out_ds[sl] = lut_relabel(d.tile(in_ds, sl), k, v).cpu().numpy().view(np.uint64)
    return out_seg


# ---- command line ----

@click.group()
def utils():
    """Utility functions for volumes and segmentations"""


def _cmd(name, fn, options):
    f = lambda **kw: fn(**kw)  # noqa: E731
    f.__doc__ = fn.__doc__ or name
    for opt in reversed(options):
        f = opt(f)
    return utils.command(name)(f)


_in = click.option("--in_array", "-i", type=click.Path(exists=True), required=True, help="The path of the input zarr array")
_out = click.option("--out_array", "-o", type=click.Path(), help="The path of the output zarr array")
_cmd("mask", mask, [_in, _out, click.option("--mode", "-m", type=click.Choice(["raw", "labels"]), required=True,
                                            help="Specify whether to mask image or objects")])
_cmd("scale_pyramid", scale_pyramid, [
    click.option("--in_array", "-i", type=click.Path(exists=True), required=True,
                 help="The path of the input zarr array, which may already end in a scale level"),
    click.option("--scales", "-s", multiple=True, required=True, type=str, help="Spatial scale factors for one level, e.g. 2,2,2. Repeat per level"),
    click.option("--chunk_shape", "-c", type=str, default=None, help="Spatial chunk shape in voxels, e.g. 64,64,64. Defaults to the input's"),
    click.option("--mode", "-m", type=click.Choice(["up", "down"]), required=True, help="Upscale or downscale")])
_cmd("bbox", bbox, [_in, _out, click.option("--padding", "-p", type=int, default=0, help="Padding to add to the bounding box.")])
_cmd("merge", merge, [
    click.option("--in_seg", "-i", type=click.Path(exists=True), required=True, help="The path of the input segmentation zarr array"),
    click.option("--out_seg", "-o", type=click.Path(), help="The path of the output segmentation zarr array"),
    click.option("--luts", "-l", type=click.Path(exists=True), required=True, help="Path to the LUTs file")])
