"""Minimal Zarr v2 directory-store arrays with the funlib.persistence metadata convention.

The reference reads and writes volumes through `funlib.persistence.open_ds / prepare_ds`
(/root/reference/bootstrapper/predict.py:169-178, post/watershed.py:319-330) on top of zarr-python;
neither package exists on the GPU box, so this module implements the on-disk format directly:
`.zarray` / `.zattrs` JSON, C-order chunks named by `dimension_separator`, and the numcodecs
compressors null / zlib / gzip / zstd / lz4 / blosc (lz4, lz4hc, zstd, zlib, blosclz frames; byte
and bit shuffle) through libbsmi's chunk codecs (include/bsmi_io.h), which decode and encode the
chunks of one request on a pool of host threads.  New arrays get zarr-python's default compressor
(Blosc lz4, clevel 5, byte shuffle), as they do in the reference.  Attributes follow
funlib.persistence: `offset`, `voxel_size` (alias `resolution`), `axis_names`, `units`; a leading
channel axis is named "c^".
"""
import json
import os

import numpy as np

from . import codecs

def _default_threads():
    """native threads of one read / write request: the cores this process may use, at most 32 (a GPU's share of a node's host
    cores; `bs segment` keeps a few requests in flight, each on its own set)"""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 8
    return max(4, min(32, n))


IO_THREADS = int(os.environ.get("BSMI_IO_THREADS", "0")) or _default_threads()


def split_store(path):
    """'/a/b.zarr/x/y' -> ('/a/b.zarr', 'x/y')"""
    marker = ".zarr"
    i = path.rfind(marker)
    if i < 0:
        raise ValueError(f"{path!r} does not point into a .zarr container")
    container = path[: i + len(marker)]
    return container, path[i + len(marker):].strip("/")


class ZarrArray:
    def __init__(self, path, mode="r"):
        self.path = path.rstrip("/")
        self.mode = mode
        zarray = os.path.join(self.path, ".zarray")
        if not os.path.exists(zarray):
            raise FileNotFoundError(f"no zarr array at {self.path}")
        with open(zarray) as f:
            self.meta = json.load(f)
        if self.meta.get("zarr_format") != 2:
            raise ValueError("only zarr format 2 is supported")
        if self.meta.get("order", "C") != "C":
            raise ValueError("only C-order zarr arrays are supported")
        if self.meta.get("filters"):
            raise ValueError("zarr filters are not supported")
        self.shape = tuple(self.meta["shape"])
        self.chunks = tuple(self.meta["chunks"])
        self.dtype = np.dtype(self.meta["dtype"])
        self.fill_value = self.meta.get("fill_value") or 0
        self.sep = self.meta.get("dimension_separator", ".")
        comp = self.meta.get("compressor")
        self.compressor = None if comp is None else comp.get("id")
        self.codec = codecs.from_config(comp, self.dtype.itemsize)
        self.chunk_nbytes = int(np.prod(self.chunks)) * self.dtype.itemsize
        self.attrs = {}
        za = os.path.join(self.path, ".zattrs")
        if os.path.exists(za):
            with open(za) as f:
                self.attrs = json.load(f)

    # -- funlib.persistence style metadata -----------------------------------------------
    @property
    def spatial_dims(self):
        return len(self.voxel_size)

    @property
    def voxel_size(self):
        v = self.attrs.get("voxel_size", self.attrs.get("resolution"))
        if v is None:
            nd = min(3, len(self.shape))
            v = [1] * nd
        return tuple(int(x) for x in v)

    @property
    def offset(self):
        o = self.attrs.get("offset")
        if o is None:
            o = [0] * len(self.voxel_size)
        return tuple(int(x) for x in o)

    @property
    def axis_names(self):
        names = self.attrs.get("axis_names")
        if names is None:
            nd = len(self.voxel_size)
            names = ["c^"] * (len(self.shape) - nd) + ["z", "y", "x"][-nd:]
        return list(names)

    @property
    def units(self):
        return list(self.attrs.get("units", [""] * len(self.voxel_size)))

    @property
    def roi(self):
        """(offset, shape) of the spatial extent in world units."""
        nd = len(self.voxel_size)
        return self.offset, tuple(s * v for s, v in zip(self.shape[-nd:], self.voxel_size))

    def set_attr(self, key, value):
        if self.mode == "r":
            raise PermissionError("array opened read-only")
        self.attrs[key] = value
        with open(os.path.join(self.path, ".zattrs"), "w") as f:
            json.dump(self.attrs, f, indent=1)

    # -- chunk I/O ---------------------------------------------------------------------------
    def _chunk_path(self, idx):
        return os.path.join(self.path, self.sep.join(str(i) for i in idx))

    def _read_chunks(self, idxs):
        """Chunks `idxs` (grid indices), read and decoded side by side; missing files are fill_value chunks."""
        bufs = codecs.read_chunks(self.codec, [self._chunk_path(i) for i in idxs], self.chunk_nbytes, IO_THREADS)
        out = []
        for b in bufs:
            if b is None:
                out.append(np.full(self.chunks, self.fill_value, dtype=self.dtype))
            else:
                out.append(b.view(self.dtype).reshape(self.chunks))
        return out

    def _write_chunks(self, idxs, arrays):
        paths = [self._chunk_path(i) for i in idxs]
        for d in {os.path.dirname(p) for p in paths}:
            os.makedirs(d, exist_ok=True)
        codecs.write_chunks(self.codec, paths, [np.ascontiguousarray(a, dtype=self.dtype) for a in arrays], IO_THREADS)

    def _norm(self, key):
        if not isinstance(key, tuple):
            key = (key,)
        key = key + (slice(None),) * (len(self.shape) - len(key))
        out = []
        for k, n in zip(key, self.shape):
            if not isinstance(k, slice) or k.step not in (None, 1):
                raise IndexError("only contiguous slices are supported")
            a, b, _ = k.indices(n)
            out.append((a, max(a, b)))
        return out

    def _chunk_grid(self, box):
        ranges = [range(a // c, (b - 1) // c + 1) if b > a else range(0) for (a, b), c in zip(box, self.chunks)]
        return [tuple(r[i] for r, i in zip(ranges, idx)) for idx in np.ndindex(*[len(r) for r in ranges])]

    def _overlap(self, box, cidx):
        """(slices inside the chunk, slices inside the box, does the box cover the chunk's valid extent)"""
        inner, outer, covers = [], [], True
        for (a, b), c, ci, n in zip(box, self.chunks, cidx, self.shape):
            lo, hi = max(a, ci * c), min(b, (ci + 1) * c)
            inner.append(slice(lo - ci * c, hi - ci * c))
            outer.append(slice(lo - a, hi - a))
            covers &= lo == ci * c and hi == min((ci + 1) * c, n)
        return tuple(inner), tuple(outer), covers

    def _copies(self, box, host, rmw):
        """the chunks under `box` as bsmi_chunk_copy records against the host array `host` (shape = the box's extents)"""
        import ctypes as C
        from . import _lib
        nd = len(self.shape)
        grid = self._chunk_grid(box)
        arr = (_lib.ChunkCopy * max(1, len(grid)))()
        pad = 4 - nd
        item = self.dtype.itemsize
        paths = []
        for rec, cidx in zip(arr, grid):
            inner, outer, covers = self._overlap(box, cidx)
            p = self._chunk_path(cidx).encode()
            paths.append(p)
            rec.path = p
            off = sum(o.start * st for o, st in zip(outer, host.strides))
            rec.base = host.ctypes.data + off
            for d in range(4):
                if d < pad:
                    rec.start[d], rec.extent[d], rec.stride[d] = 0, 1, 0
                else:
                    sl = inner[d - pad]
                    rec.start[d], rec.extent[d], rec.stride[d] = sl.start, sl.stop - sl.start, host.strides[d - pad]
            rec.stride[3] = item
            rec.read_modify_write = 1 if (rmw and not covers) else 0
        cs = (C.c_int64 * 4)(*([1] * pad + list(self.chunks)))
        return arr, grid, cs, paths

    def _fill_bytes(self):
        return np.asarray(self.fill_value, dtype=self.dtype).tobytes()

    def read_into(self, key, out):
        """self[key] -> the host array `out` (numpy, shape of the selection, last axis contiguous; e.g. a view of page-locked
        memory), decoded and copied by the library's threads chunk by chunk (no chunk-sized arrays in the interpreter).  A
        selection that stops before a chunk's last leading index (three of six channels) decodes only that part of a Blosc chunk."""
        import ctypes as C
        from . import _lib
        box = self._norm(key)
        shape = tuple(b - a for a, b in box)
        if tuple(out.shape) != shape or out.dtype != self.dtype:
            raise ValueError(f"read_into: destination {out.shape} {out.dtype}, selection {shape} {self.dtype}")
        if len(self.shape) > 4 or (out.ndim and out.strides[-1] != self.dtype.itemsize) or not out.flags.writeable:
            out[...] = self._getitem_python(box)
            return out
        if out.size == 0:
            return out
        arr, grid, cs, _paths = self._copies(box, out, False)
        status = (C.c_int * len(grid))()
        fill = self._fill_bytes()
        _lib.check(_lib.lib.bsmi_chunks_read_into(C.byref(self.codec), len(grid), arr, cs, self.dtype.itemsize,
                                                  C.c_char_p(fill), status, IO_THREADS))
        return out

    def write_from(self, key, src):
        """self[key] = src (numpy, shape of the selection, last axis contiguous): rows gathered, chunks encoded and written by the
        library's threads; chunks the selection covers only partly are read back first (inside the same threads)."""
        import ctypes as C
        from . import _lib
        if self.mode == "r":
            raise PermissionError("array opened read-only")
        box = self._norm(key)
        shape = tuple(b - a for a, b in box)
        if tuple(src.shape) != shape or src.dtype != self.dtype or len(self.shape) > 4 or (src.ndim and src.strides[-1] != self.dtype.itemsize) \
                or any(st < 0 for st in src.strides) or (src.ndim and 0 in src.strides[:-1] and src.size > shape[-1]):
            src = np.ascontiguousarray(np.broadcast_to(np.asarray(src, dtype=self.dtype), shape))
        if src.size == 0:
            return
        if len(self.shape) > 4:   # the library's chunk copies have four axes (a stacked 2-D snapshot has five)
            self._setitem_python(box, src)
            return
        arr, grid, cs, paths = self._copies(box, src, True)
        for d in {os.path.dirname(p) for p in paths}:
            os.makedirs(d, exist_ok=True)
        status = (C.c_int * len(grid))()
        fill = self._fill_bytes()
        _lib.check(_lib.lib.bsmi_chunks_write_from(C.byref(self.codec), len(grid), arr, cs, self.dtype.itemsize,
                                                   C.c_char_p(fill), status, IO_THREADS))

    def _getitem_python(self, box):
        out = np.empty([b - a for a, b in box], dtype=self.dtype)
        grid = self._chunk_grid(box)
        for cidx, chunk in zip(grid, self._read_chunks(grid)):
            inner, outer, _ = self._overlap(box, cidx)
            out[outer] = chunk[inner]
        return out

    def _setitem_python(self, box, src):
        grid = self._chunk_grid(box)
        chunks = []
        for cidx in grid:
            inner, outer, covers = self._overlap(box, cidx)
            chunk = np.full(self.chunks, self.fill_value, dtype=self.dtype) if covers else self._read_chunks([cidx])[0].copy()
            chunk[inner] = src[outer]
            chunks.append(chunk)
        self._write_chunks(grid, chunks)

    def __getitem__(self, key):
        box = self._norm(key)
        return self.read_into(key, np.empty([b - a for a, b in box], dtype=self.dtype))

    def __setitem__(self, key, value):
        if self.mode == "r":
            raise PermissionError("array opened read-only")
        box = self._norm(key)
        shape = [b - a for a, b in box]
        v = np.asarray(value, dtype=self.dtype)
        if list(v.shape) != shape:
            v = np.ascontiguousarray(np.broadcast_to(v, shape))
        self.write_from(key, v)

    # -- world-unit ROI access ------------------------------------------------------------------
    def roi_to_slices(self, roi_offset, roi_shape):
        nd = len(self.voxel_size)
        sl = []
        for o, s, off, v in zip(roi_offset, roi_shape, self.offset, self.voxel_size):
            if (o - off) % v or s % v:
                raise ValueError("ROI is not aligned to the voxel grid")
            sl.append(slice((o - off) // v, (o - off + s) // v))
        return (slice(None),) * (len(self.shape) - nd) + tuple(sl)


def open_ds(path, mode="r"):
    return ZarrArray(path, mode)


def _ensure_groups(container, dataset):
    os.makedirs(container, exist_ok=True)
    g = os.path.join(container, ".zgroup")
    if not os.path.exists(g):
        with open(g, "w") as f:
            json.dump({"zarr_format": 2}, f)
    cur = container
    parts = [p for p in dataset.split("/") if p]
    for p in parts[:-1]:
        cur = os.path.join(cur, p)
        os.makedirs(cur, exist_ok=True)
        g = os.path.join(cur, ".zgroup")
        if not os.path.exists(g):
            with open(g, "w") as f:
                json.dump({"zarr_format": 2}, f)


def _compressor_config(compressor):
    if compressor is None:
        return None
    if isinstance(compressor, dict):
        return dict(compressor)
    if compressor in ("default", "blosc"):
        return dict(codecs.DEFAULT_COMPRESSOR)
    if compressor == "lz4":
        return {"id": "lz4", "acceleration": 1}
    if compressor in ("zstd", "zlib", "gzip"):
        return {"id": compressor, "level": 1}
    raise NotImplementedError(f"zarr compressor {compressor!r} is not supported")


def prepare_ds(store, shape, offset=None, voxel_size=None, axis_names=None, units=None, chunk_shape=None,
               dtype=np.uint8, compressor="default", mode="w"):
    """Create (or overwrite) a dataset with funlib.persistence-style attributes and open it r+.
    compressor: "default" (zarr-python's Blosc lz4 / clevel 5 / byte shuffle), None (raw chunks), a codec
    name ("zstd", "zlib", "gzip", "lz4", "blosc") or a numcodecs config dict."""
    container, dataset = split_store(store)
    _ensure_groups(container, dataset)
    path = os.path.join(container, dataset)
    if os.path.exists(os.path.join(path, ".zarray")) and mode == "w":
        for name in os.listdir(path):
            fp = os.path.join(path, name)
            if os.path.isfile(fp):
                os.remove(fp)
    os.makedirs(path, exist_ok=True)
    shape = [int(s) for s in shape]
    chunks = [int(c) for c in (chunk_shape or shape)]
    chunks = [max(1, min(c, s)) if s > 0 else 1 for c, s in zip(chunks, shape)]
    dt = np.dtype(dtype)
    meta = {
        "zarr_format": 2, "shape": shape, "chunks": chunks,
        "dtype": dt.str if dt.itemsize > 1 else "|" + dt.str[1:], "fill_value": 0, "order": "C", "filters": None,
        "dimension_separator": ".",
        "compressor": _compressor_config(compressor),
    }
    with open(os.path.join(path, ".zarray"), "w") as f:
        json.dump(meta, f, indent=1)
    nd = len(voxel_size) if voxel_size is not None else min(3, len(shape))
    attrs = {
        "offset": [int(o) for o in (offset if offset is not None else [0] * nd)],
        "voxel_size": [int(v) for v in (voxel_size if voxel_size is not None else [1] * nd)],
    }
    if axis_names is not None:
        attrs["axis_names"] = list(axis_names)
    if units is not None:
        attrs["units"] = list(units)
    with open(os.path.join(path, ".zattrs"), "w") as f:
        json.dump(attrs, f, indent=1)
    return ZarrArray(path, "r+")
