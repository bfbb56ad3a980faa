"""Synthetic labels for the second-stage setups (`3d_affs_from_*`): the draw plan, the structuring bitmaps and the
wrappers around csrc/synth.hip.

Reference being mirrored (paths relative to /root/reference/bootstrapper):
  gp/create_labels.py:98-179      _generate_labels: tubes / random branch, black-out, every anisotropy-th section
  gp/custom_grow_boundary.py      only_xy=True, no mask
  gp/obfuscate_labels.py          _generate_operations, split / merge / artifact

All host draws come from ONE `random.Random(seed)` stream in the reference's order of draws (the reference mixes the
`random` module with `np.random` for the noise volume and the black-out flags; here the flags come from the same stream and
the noise from `torch.rand` on the device, seeded by a draw of that stream).  The device rules -- where scipy / skimage
leave a choice open, the one made here -- are written out in include/bsmi.h, DESIGN.md section 7i and tests/synth_ref.py.
The bitmaps restate skimage.morphology's star / disk / ellipse and scipy's generate_binary_structure(2, k); skimage is
not installed where this was written, so their parity is unpinned until tools/gen_goldens_synth.py has been run
(tests/test_synth_pin.py).
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib

GAUSS_SIGMA, GAUSS_RADIUS, PEAK_WINDOW = 10.0, 40, 15   # gaussian_filter(sigma=10) truncates at 4 sigma; maximum_filter(peaks, 15)
_M64 = (1 << 64) - 1


# ---- structuring bitmaps ----

def star(a):
    """skimage.morphology.star(a): a square of side 2a + 1 and its 45-degree rotation (the diamond |dy| + |dx| <= c)
    on a grid of side 2a + 1 + 2 (a // 2)."""
    a = int(a)
    if a == 1:
        return np.ones((3, 3), dtype=bool)
    m, n = 2 * a + 1, a // 2
    size = m + 2 * n
    c = (size - 1) // 2
    out = np.zeros((size, size), dtype=bool)
    out[n:m + n, n:m + n] = True
    yy, xx = np.mgrid[:size, :size]
    out |= (np.abs(yy - c) + np.abs(xx - c)) <= c
    return out


def disk(r):
    """skimage.morphology.disk(r): dy^2 + dx^2 <= r^2 on a grid of side 2r + 1."""
    r = int(r)
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return (yy * yy + xx * xx) <= r * r


def ellipse(width, height):
    """skimage.morphology.ellipse(width, height): (dy / (height + 1))^2 + (dx / (width + 1))^2 < 1 on a grid of
    (2 height + 1, 2 width + 1) -- skimage.draw.ellipse with radii one larger than the half-axes."""
    w, h = int(width), int(height)
    yy, xx = np.mgrid[-h:h + 1, -w:w + 1]
    return (yy / (h + 1.0)) ** 2 + (xx / (w + 1.0)) ** 2 < 1.0


def binary_structure(k):
    """scipy.ndimage.generate_binary_structure(2, k): the cross (k = 1) or the full 3 x 3 (k = 2)."""
    yy, xx = np.mgrid[-1:2, -1:2]
    return (np.abs(yy) + np.abs(xx)) <= int(k)


def pack_bitmap(struct):
    """bool (h, w), both <= 32 -> (uint32 [32], h, w): bit c of word r = struct[r, c]."""
    s = np.asarray(struct, dtype=bool)
    h, w = s.shape
    if not (1 <= h <= 32 and 1 <= w <= 32):
        raise ValueError(f"a structuring bitmap is at most 32 x 32, not {h} x {w}")
    rows = np.zeros(32, dtype=np.uint32)
    rows[:h] = (s.astype(np.uint64) << np.arange(w, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)
    return rows, h, w


# ---- the draw plan ----

@dataclass
class LabelPlan:
    """Every host draw of one CreateLabels sample.  `shape` is the volume asked for; the generated volume has
    anisotropy * shape[0] sections."""
    shape: tuple
    anisotropy: int
    choice: str                       # "tubes" | "random"
    radii: tuple                      # the seven radius draws of create_labels.py:107-115
    structs: list = field(repr=False, default_factory=list)
    points: np.ndarray = None         # tubes: int32 (n, 3)
    dilations: np.ndarray = None      # tubes: int32 (sections,) 1..10
    struct_index: np.ndarray = None   # tubes: int32 (sections,) into structs
    noise_seed: int = 0               # random: seed of the device's noise volume
    drop3: bool = False
    drop5: bool = False

    @property
    def generated_shape(self):
        return (self.shape[0] * self.anisotropy, self.shape[1], self.shape[2])


def anisotropy_range(voxel_size):
    """CreateLabels.setup: (2, max(4, int(voxel_size[0] / voxel_size[1])))"""
    return (2, max(4, int(voxel_size[0] / voxel_size[1])))


def draw_plan(rng, shape, aniso_range):
    """create_labels.py:98-177 in its order of draws."""
    shape = tuple(int(v) for v in shape)
    anisotropy = rng.randint(*aniso_range)
    gen = (shape[0] * anisotropy, shape[1], shape[2])
    choice = rng.choice(["tubes", "random"])
    r = [rng.randint(4, 6), rng.randint(3, 5), rng.randint(1, 4), rng.randint(2, 4), rng.randint(2, 4), rng.randint(2, 4), rng.randint(6, 8)]
    structs = [star(r[0]), binary_structure(2), star(r[1]), disk(r[2]), star(r[3]), ellipse(r[4], r[5]), star(r[6])]
    plan = LabelPlan(shape=shape, anisotropy=anisotropy, choice=choice, radii=tuple(r), structs=structs)
    if choice == "tubes":
        n = rng.randint(5, 5 * anisotropy)
        plan.points = np.array([[rng.randint(1, gen[0] - 1), rng.randint(1, gen[1] - 1), rng.randint(1, gen[2] - 1)] for _ in range(n)],
                               dtype=np.int32).reshape(n, 3)
        dil, idx = [], []
        for _ in range(gen[0]):
            dil.append(rng.randint(1, 10))
            idx.append(rng.randrange(len(structs)))   # random.choice(structs)
        plan.dilations, plan.struct_index = np.array(dil, dtype=np.int32), np.array(idx, dtype=np.int32)
    else:
        plan.noise_seed = rng.getrandbits(63)
    plan.drop3 = rng.random() < 0.2
    plan.drop5 = rng.random() < 0.2
    return plan


def draw_operations(rng, num_tries=5, p_split=0.1, p_merge=0.1, p_artifact=0.1):
    """obfuscate_labels.py:76-86: ONE r per try, compared against all three probabilities."""
    ops = []
    for _ in range(num_tries):
        r = rng.random()
        if r < p_split:
            ops.append("split")
        if r < p_merge:
            ops.append("merge")
        if r < p_artifact:
            ops.append("artifact")
    return ops


def mix64(k):
    k &= _M64
    k ^= k >> 33
    k = k * 0xff51afd7ed558ccd & _M64
    k ^= k >> 33
    k = k * 0xc4ceb9fe1a85ec53 & _M64
    k ^= k >> 33
    return k


def grow_steps(seed, z, label, max_steps):
    """steps of CustomGrowBoundary for (section, label): the counter hash of csrc/synth.hip (synth_steps)"""
    return mix64(mix64(mix64(seed) ^ z) ^ (label & _M64)) % (max_steps + 1)


def gaussian_weights(sigma=GAUSS_SIGMA, radius=GAUSS_RADIUS):
    """scipy.ndimage._gaussian_kernel1d(sigma, 0, radius) in float64"""
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (sigma * sigma) * x * x)
    return phi / phi.sum()


# ---- the wrappers ----

def _ptr(t):
    return C.c_void_p(t.data_ptr())


class SynthEngine:
    """Work space of csrc/synth.hip for generated volumes of up to `max_shape`; one per host thread and GPU."""

    def __init__(self, max_shape, device=0):
        self.dev = torch.device("cuda", device)
        self.max_shape = tuple(int(v) for v in max_shape)
        h = C.c_void_p()
        _lib.check(_lib.lib.bsmi_synth_create(self.dev.index, _lib.i64x3(self.max_shape), C.byref(h)))
        self._h = h

    def close(self):
        if self._h is not None:
            _lib.lib.bsmi_synth_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def _check(self, t, dtype, name):
        if t.dtype != dtype or not t.is_cuda or t.dim() != 3 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtype} CUDA tensor (D, H, W)")

    def dilate_points(self, shape, points, structs, struct_index, iterations):
        """int32 0 / 1 volume of the dilated points; section z uses structs[struct_index[z]], iterations[z] times"""
        shape = tuple(int(v) for v in shape)
        d = shape[0]
        packed = [pack_bitmap(s) for s in structs]
        bm = np.zeros((d, 32), dtype=np.uint32)
        sz = np.zeros((d, 2), dtype=np.int32)
        for z in range(d):
            rows, h, w = packed[int(struct_index[z])]
            bm[z], sz[z] = rows, (h, w)
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.int32).reshape(-1, 3))
        its = np.ascontiguousarray(np.asarray(iterations, dtype=np.int32))
        if its.shape != (d,):
            raise ValueError("one iteration count per section")
        out = torch.empty(shape, dtype=torch.int32, device=self.dev)
        _lib.check(_lib.lib.bsmi_synth_dilate_points(self._h, _lib.i64x3(shape), pts.ctypes.data_as(C.c_void_p), len(pts),
                                                     bm.ctypes.data_as(C.c_void_p), sz.ctypes.data_as(C.c_void_p), its.ctypes.data_as(C.c_void_p),
                                                     _ptr(out), self._stream()))
        return out

    def label(self, vol):
        """26-connected components of equal non-zero values, raster ranks -> (int32 labels, count)"""
        self._check(vol, torch.int32, "vol")
        out, num = torch.empty_like(vol), C.c_uint64()
        _lib.check(_lib.lib.bsmi_synth_label_i32(self._h, _ptr(vol), _lib.i64x3(vol.shape), _ptr(out), C.byref(num), self._stream()))
        return out, int(num.value)

    def expand(self, labels, depth, fill):
        self._check(labels, torch.int32, "labels")
        out = torch.empty_like(labels)
        _lib.check(_lib.lib.bsmi_synth_expand_i32(self._h, _ptr(labels), _lib.i64x3(labels.shape), int(depth), int(fill), _ptr(out), self._stream()))
        return out

    def tubes(self, fg):
        self._check(fg, torch.int32, "fg")
        out, num = torch.empty_like(fg), C.c_uint64()
        _lib.check(_lib.lib.bsmi_synth_tubes_i32(self._h, _ptr(fg), _lib.i64x3(fg.shape), _ptr(out), C.byref(num), self._stream()))
        return out, int(num.value)

    def gaussian(self, vol, sigma=GAUSS_SIGMA, radius=GAUSS_RADIUS):
        self._check(vol, torch.float32, "vol")
        w = np.ascontiguousarray(gaussian_weights(sigma, radius).astype(np.float32))
        out = torch.empty_like(vol)
        _lib.check(_lib.lib.bsmi_synth_gaussian_f32(self._h, _ptr(vol), _lib.i64x3(vol.shape), w.ctypes.data_as(C.c_void_p), int(radius), _ptr(out),
                                                    self._stream()))
        return out

    def argmax_filter(self, fld, window=PEAK_WINDOW):
        self._check(fld, torch.float32, "field")
        pos = torch.empty(fld.shape, dtype=torch.int32, device=self.dev)
        _lib.check(_lib.lib.bsmi_synth_argmax_filter_f32(self._h, _ptr(fld), _lib.i64x3(fld.shape), int(window), _ptr(pos), self._stream()))
        return pos

    def basins(self, fld, pos, mask=None):
        self._check(fld, torch.float32, "field")
        self._check(pos, torch.int32, "pos")
        if pos.shape != fld.shape:
            raise ValueError("pos must have the field's shape")
        if mask is not None:
            self._check(mask, torch.uint8, "mask")
            if mask.shape != fld.shape:
                raise ValueError("mask must have the field's shape")
        out, num = torch.empty_like(pos), C.c_uint64()
        _lib.check(_lib.lib.bsmi_synth_basins_f32(self._h, _ptr(fld), _ptr(pos), _ptr(mask) if mask is not None else None, _lib.i64x3(fld.shape),
                                                  _ptr(out), C.byref(num), self._stream()))
        return out, int(num.value)

    def finish(self, labels, drop3, drop5, anisotropy):
        self._check(labels, torch.int32, "labels")
        d = int(labels.shape[0])
        a = int(anisotropy)
        dout = -(-d // a) if a <= d else 1
        out = torch.empty((dout,) + tuple(labels.shape[1:]), dtype=torch.int64, device=self.dev)
        _lib.check(_lib.lib.bsmi_synth_finish_i32(self._h, _ptr(labels), _lib.i64x3(labels.shape), int(bool(drop3)), int(bool(drop5)), a, _ptr(out),
                                                  self._stream()))
        return out

    def grow_boundary(self, labels, seed, max_steps):
        self._check(labels, torch.int64, "labels")
        out = torch.empty_like(labels)
        _lib.check(_lib.lib.bsmi_synth_grow_boundary_i64(self.dev.index, _ptr(labels), _lib.i64x3(labels.shape), C.c_uint64(int(seed) & _M64),
                                                         int(max_steps), _ptr(out), self._stream()))
        return out

    def merge(self, labels, sections, a, b):
        """in place: in `sections`, label b becomes label a"""
        self._check(labels, torch.int64, "labels")
        zs = (C.c_int32 * len(sections))(*[int(z) for z in sections])
        _lib.check(_lib.lib.bsmi_synth_merge_i64(self.dev.index, _ptr(labels), _lib.i64x3(labels.shape), zs, len(sections), int(a), int(b), self._stream()))

    def stamp(self, labels, z, y, x, struct, value):
        """in place: the set voxels of `struct`, its corner at (z, y, x), take `value`"""
        self._check(labels, torch.int64, "labels")
        rows, h, w = pack_bitmap(struct)
        _lib.check(_lib.lib.bsmi_synth_stamp_i64(self.dev.index, _ptr(labels), _lib.i64x3(labels.shape), int(z), int(y), int(x),
                                                 rows.ctypes.data_as(C.c_void_p), h, w, int(value), self._stream()))

    def present(self, labels, capacity=32768):
        """the non-zero ids present, ascending (a python list; the table is built on the device, the list read back)"""
        self._check(labels, torch.int64, "labels")
        ids = torch.empty(capacity, dtype=torch.int64, device=self.dev)
        n = C.c_uint32()
        _lib.check(_lib.lib.bsmi_synth_present_i64(self._h, _ptr(labels), labels.numel(), _ptr(ids), capacity, C.byref(n), self._stream()))
        return sorted(ids[: int(n.value)].tolist())

    def split(self, labels, label_id, window, sections, scale):
        """in place; returns the number of fragments"""
        self._check(labels, torch.int64, "labels")
        zs = (C.c_int32 * len(sections))(*[int(z) for z in sections])
        num = C.c_uint64()
        _lib.check(_lib.lib.bsmi_synth_split_i64(self._h, _ptr(labels), _lib.i64x3(labels.shape), int(label_id), int(window), zs, len(sections),
                                                 int(scale), C.byref(num), self._stream()))
        return int(num.value)

    # ---- the reference's nodes ----

    def random_labels(self, noise):
        """create_labels.py:160-167 by the specified rule: gaussian -> argmax filter -> basins"""
        peaks = self.gaussian(noise)
        return self.basins(peaks, self.argmax_filter(peaks, PEAK_WINDOW))[0]

    def create_labels(self, plan):
        """CreateLabels._generate_labels of one plan -> int64 (shape[0] or 1, H, W)"""
        gen = plan.generated_shape
        if plan.choice == "tubes":
            fg = self.dilate_points(gen, plan.points, plan.structs, plan.struct_index, plan.dilations)
            lab = self.tubes(fg)[0]
        else:
            g = torch.Generator(device=self.dev).manual_seed(int(plan.noise_seed))
            lab = self.random_labels(torch.rand(gen, generator=g, dtype=torch.float32, device=self.dev))
        return self.finish(lab, plan.drop3, plan.drop5, plan.anisotropy)

    def obfuscate(self, labels, rng, num_tries=5, p_split=0.1, p_merge=0.1, p_artifact=0.1):
        """ObfuscateLabels.process on a copy of `labels` (int64 (D, H, W)); draws from `rng` in the reference's order"""
        lab = labels.clone()
        ids = self.present(lab)
        if not ids:
            return lab
        d, h, w = (int(v) for v in lab.shape)
        for op in draw_operations(rng, num_tries, p_split, p_merge, p_artifact):
            if op == "split" and ids:
                label_id = ids[rng.randrange(len(ids))]
                window = rng.randint(15, 50)
                zs = rng.sample(range(d), k=rng.randint(1, 2))
                self.split(lab, label_id, window, zs, max(self.present(lab)))
                ids = self.present(lab)
            if op == "merge" and len(ids) >= 2:
                zs = rng.sample(range(d), k=rng.randint(1, 2))
                a, b = rng.sample(ids, 2)
                self.merge(lab, zs, a, b)
                ids = [i for i in ids if i != b]
            if op == "artifact" and ids:
                structs = [star(rng.randint(2, 8)), binary_structure(rng.randint(1, 2)), disk(rng.randint(1, 8)),
                           ellipse(rng.randint(2, 8), rng.randint(2, 8))]
                new_label = max(self.present(lab)) + 1
                for z in rng.sample(range(d), k=rng.randint(1, 2)):
                    art = structs[rng.randrange(len(structs))]
                    if art.shape[0] > h or art.shape[1] > w:
                        raise ValueError(f"sections of {h} x {w} are smaller than an artifact of {art.shape[0]} x {art.shape[1]}")
                    y, x = rng.randint(0, h - art.shape[0]), rng.randint(0, w - art.shape[1])
                    self.stamp(lab, z, y, x, art, new_label)
                    new_label += 1
        return lab
