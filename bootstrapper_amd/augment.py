"""Geometric training augmentation of 3-D samples on the device: SimpleAugment -> DeformAugment -> ShiftAugment of the
first-stage 3-D setups (reference models/3d_affs/train.py:95-104 and its 3d_lsd / 3d_mtlsd siblings), composed into ONE
coordinate map and applied by two launches of csrc/augment.hip: bsmi_aug_coords writes the source coordinate s(p) of
every voxel of the input block, bsmi_aug_sample_* resample raw (trilinear), labels and mask (nearest) through it.

These are specified rules (restated in float64 by tests/aug_ref.py), not a transcription of
gunpowder, which is not installed where this was written: parity with the reference is in distribution, not draw by
draw.  With I the input shape, c = (I - 1) / 2 and p a voxel index of the input block:

    r    = p + (0, sh_y[p_z], sh_x[p_z])     ShiftAugment: integer shift per section
    t    = A (r - c) + E(r)                  DeformAugment: A = u Rz(theta), E = trilinear elastic displacement
    s(p) = c_src + M t                       SimpleAugment: y <-> x swap, then the mirrors; c_src = c in the crop's voxels

Declared differences: E is evaluated at every voxel (the reference's subsample=4 is a CPU shortcut); the 5 % rejection
test sees the augmented output block (gunpowder's Reject sees the upstream region); rotations are about z only.
NOT built: the intensity nodes (NoiseAugment, IntensityAugment, GammaAugment, ImpulseNoiseAugment, SmoothAugment,
DefectAugment), the 2-D setups, SyntheticSource, 3-D rotations.
"""
import ctypes as C
import dataclasses
import math

import numpy as np

NOT_BUILT = "NoiseAugment, IntensityAugment, GammaAugment, ImpulseNoiseAugment, SmoothAugment and DefectAugment of raw"
MAX_LATTICE_NODES = 4096   # csrc/augment.hip: 48 KiB of offsets in LDS


@dataclasses.dataclass(frozen=True)
class AugParams:
    """The arguments of the three nodes; the defaults are the reference's (models/3d_affs/train.py:95-104).
    control_point_spacing / jitter_sigma: world units per axis, None = the reference's voxel_size * (vs[2], vs[0], vs[0])
    and voxel_size * 2."""
    simple: bool = True
    deform_p: float = 0.5
    scale_interval: tuple = (0.9, 1.1)
    rotate: bool = True
    control_point_spacing: tuple = None
    jitter_sigma: tuple = None
    shift_p: float = 0.5
    prob_slip: float = 0.2
    prob_shift: float = 0.2
    shift_sigma: float = 3.0

    @classmethod
    def from_config(cls, value):
        """The train TOML key `augment`: absent / false -> None (today's path), true -> the defaults, a table -> overrides."""
        if value is None or value is False:
            return None
        if value is True:
            return cls()
        if not isinstance(value, dict):
            raise ValueError(f"augment must be true, false or a table, not {value!r}")
        names = [f.name for f in dataclasses.fields(cls)]
        unknown = sorted(set(value) - set(names))
        if unknown:
            raise ValueError(f"unknown augment key(s) {', '.join(unknown)}; known: {', '.join(names)}")
        kw = {}
        for k, v in value.items():
            if k in ("simple", "rotate"):
                kw[k] = bool(v)
            elif k == "scale_interval":
                kw[k] = tuple(float(x) for x in v)
                if len(kw[k]) != 2 or not 0 < kw[k][0] <= kw[k][1]:
                    raise ValueError(f"augment.scale_interval {v!r}: two positive numbers, low <= high")
            elif k in ("control_point_spacing", "jitter_sigma"):
                kw[k] = tuple(float(x) for x in v)
                if len(kw[k]) != 3 or (k == "control_point_spacing" and min(kw[k]) <= 0) or min(kw[k]) < 0:
                    raise ValueError(f"augment.{k} {v!r}: three world-unit values (z, y, x)")
            else:
                kw[k] = float(v)
                if kw[k] < 0 or (k != "shift_sigma" and kw[k] > 1):
                    raise ValueError(f"augment.{k} {v!r}: " + ("not negative" if k == "shift_sigma" else "a probability"))
        return cls(**kw)


@dataclasses.dataclass
class AugPlan:
    """One sample's draws, held in the number formats the kernel reads (float32 / int32), so that the float64
    restatement starts from the same numbers.  shape: I.  mirror: 3 flags (z, y, x).  swap: y <-> x.  u, theta: what was
    drawn; linear: float32 [5] = u * (1, cos, -sin, sin, cos).  lattice: float32 [3, nz, ny, nx] control offsets in voxels
    (component z, y, x) or None; inv_spacing: float32 [3], 1 / (node spacing in voxels).  shifts: int32 [2, D] (y, x per
    section) or None."""
    shape: tuple
    mirror: tuple = (False, False, False)
    swap: bool = False
    u: float = 1.0
    theta: float = 0.0
    linear: np.ndarray = None
    lattice: np.ndarray = None
    inv_spacing: np.ndarray = None
    shifts: np.ndarray = None

    def __post_init__(self):
        self.shape = tuple(int(v) for v in self.shape)
        if self.linear is None:
            self.linear = linear_of(self.u, self.theta)


def linear_of(u, theta):
    """float32 (l0 .. l4) = u * (1, cos, -sin, sin, cos): t_z = l0 d_z, t_y = l1 d_y + l2 d_x, t_x = l3 d_y + l4 d_x"""
    c, s = math.cos(theta), math.sin(theta)
    return np.array([u, u * c, -u * s, u * s, u * c], dtype=np.float32)


def lattice_shape(shape, spacing):
    """Nodes per axis of a lattice with `spacing` voxels between nodes: the block [0, I - 1] plus one node on each side --
    node k at (k - 1) * spacing, k = 0 .. ceil((I - 1) / spacing) + 2 -- and a single node on an axis of one voxel."""
    return tuple(1 if i == 1 else int(math.ceil((i - 1) / sp)) + 3 for i, sp in zip(shape, spacing))


def check_square(inp, out):
    if inp[1] != inp[2] or out[1] != out[2]:
        raise ValueError(f"the y/x swap of SimpleAugment (transpose_only=[1, 2]) needs square blocks, not input {list(inp)} / output {list(out)}; "
                         "set augment.simple = false")


def draw_plan(rng, params, shape, voxel_size):
    """One plan for a block of `shape`, every draw taken from `rng` (a numpy Generator: the sample source's own stream) in
    this order; a node whose probability is 0 or that is switched off takes no draw at all.
      1. simple:  4 x rng.random() < 0.5 -- mirror z, mirror y, mirror x, swap y/x
      2. deform:  rng.random() < deform_p; if applied: u = rng.uniform(*scale_interval); theta = rng.uniform(0, 2 pi)
                  (only when rotate); the lattice, rng.standard_normal((3, nz, ny, nx)) * sigma (voxels) per component
      3. shift:   rng.random() < shift_p; if applied: rng.random(D) < prob_shift, rint(rng.normal(0, sigma, (D, 2))) --
                  added to this section and all later ones; rng.random(D) < prob_slip, rint(rng.normal(0, sigma, (D, 2)))
                  -- added to this section alone.
    """
    shape = tuple(int(v) for v in shape)
    vs = [float(v) for v in voxel_size]
    plan = AugPlan(shape)
    if params.simple:
        if shape[1] != shape[2]:
            check_square(shape, shape)
        flags = [bool(rng.random() < 0.5) for _ in range(4)]
        plan.mirror, plan.swap = tuple(flags[:3]), flags[3]
    if params.deform_p > 0 and rng.random() < params.deform_p:
        if params.rotate and vs[1] != vs[2]:
            raise NotImplementedError(f"rotation about z needs voxel_size[1] == voxel_size[2], not {vs}; set augment.rotate = false "
                                      "(full 3-D rotations are not built)")
        plan.u = float(rng.uniform(*params.scale_interval))
        plan.theta = float(rng.uniform(0.0, 2.0 * math.pi)) if params.rotate else 0.0
        plan.linear = linear_of(plan.u, plan.theta)
        cps = params.control_point_spacing or (vs[0] * vs[2], vs[1] * vs[0], vs[2] * vs[0])
        sig = params.jitter_sigma or (2.0 * vs[0], 2.0 * vs[1], 2.0 * vs[2])
        spacing = [c / v for c, v in zip(cps, vs)]
        n = lattice_shape(shape, spacing)
        if n[0] * n[1] * n[2] > MAX_LATTICE_NODES:
            raise ValueError(f"control lattice of {n} nodes for a block of {list(shape)} at spacing {spacing} voxels: at most {MAX_LATTICE_NODES}")
        sv = np.array([s / v for s, v in zip(sig, vs)]).reshape(3, 1, 1, 1)
        plan.lattice = (rng.standard_normal((3,) + n) * sv).astype(np.float32)
        plan.inv_spacing = np.array([1.0 / sp for sp in spacing], dtype=np.float32)
    if params.shift_p > 0 and rng.random() < params.shift_p:
        d = shape[0]
        on = rng.random(d) < params.prob_shift
        step = np.rint(rng.normal(0.0, params.shift_sigma, (d, 2)))
        slip_on = rng.random(d) < params.prob_slip
        slip = np.rint(rng.normal(0.0, params.shift_sigma, (d, 2)))
        total = np.cumsum(step * on[:, None], axis=0) + slip * slip_on[:, None]
        plan.shifts = np.ascontiguousarray(total.T).astype(np.int32)
    return plan


def _interval_mul(k, lo, hi):
    return (k * lo, k * hi) if k >= 0 else (k * hi, k * lo)


def source_box(plan, region=None):
    """(lo, hi): an integer box, in voxels relative to the block's origin, hi exclusive, that contains s(p) -- taken with
    c_src = c -- and its trilinear neighbour floor(s) + 1 for every voxel p of `region` ((offset, shape) inside the block;
    default: the whole block).  The crop read for a sample is this box, so c_src = c - lo.

    The bound, by interval arithmetic on the map.  Per axis, r_a - c_a lies in [o_a - c_a + min sh_a, o_a + n_a - 1 - c_a +
    max sh_a] (sh = 0 on z).  A (r - c) is linear, so each component lies in the sum of the intervals l_k * [lo, hi] of its
    terms.  E(r) is a trilinear, i.e. convex, combination of lattice offsets (the lattice coordinate is clamped to the
    lattice), so |E_a| <= max |lattice[a]|.  The swap exchanges the y and x intervals, a mirror negates one.  That bounds
    the exact map; the kernel's float32 result differs from it by far less than a voxel (tests/aug_ref.py: coords_gate), so
    one voxel of margin below and, with the neighbour floor(s) + 1, two above make the box safe.  It is conservative: the
    corners of the interval box need not be reached (a rotated square is bounded by its own bounding square)."""
    shape = plan.shape
    off, n = ((0, 0, 0), shape) if region is None else (tuple(region[0]), tuple(region[1]))
    lin = [float(v) for v in plan.linear]
    d = []
    for a in range(3):
        c = (shape[a] - 1) / 2.0
        s_lo = s_hi = 0
        if a > 0 and plan.shifts is not None:
            zs = plan.shifts[a - 1, off[0]:off[0] + n[0]]
            s_lo, s_hi = int(zs.min()), int(zs.max())
        d.append((off[a] - c + s_lo, off[a] + n[a] - 1 - c + s_hi))
    emax = [float(np.abs(plan.lattice[a]).max()) for a in range(3)] if plan.lattice is not None else [0.0, 0.0, 0.0]

    def add(*ivs):
        return sum(i[0] for i in ivs), sum(i[1] for i in ivs)
    t = [add(_interval_mul(lin[0], *d[0]), (-emax[0], emax[0])),
         add(_interval_mul(lin[1], *d[1]), _interval_mul(lin[2], *d[2]), (-emax[1], emax[1])),
         add(_interval_mul(lin[3], *d[1]), _interval_mul(lin[4], *d[2]), (-emax[2], emax[2]))]
    if plan.swap:
        t[1], t[2] = t[2], t[1]
    lo, hi = [], []
    for a in range(3):
        a_lo, a_hi = (-t[a][1], -t[a][0]) if plan.mirror[a] else t[a]
        c = (shape[a] - 1) / 2.0
        lo.append(int(math.floor(c + a_lo)) - 1)
        hi.append(int(math.ceil(c + a_hi)) + 3)
    return tuple(lo), tuple(hi)


# ---- device wrappers (libbsmi: include/bsmi.h, "training augmentation") ----

def _f32(v):
    return (C.c_float * len(v))(*[float(x) for x in v])


def coords(plan, box_lo, device=0):
    """s(p) of every voxel of the block, in voxels of the crop whose origin lies at `box_lo` (source_box(plan)[0]) relative
    to the block: float32 CUDA (3, D, H, W)."""
    import torch
    from . import _lib
    dev = torch.device("cuda", device) if not isinstance(device, torch.device) else device
    shape = plan.shape
    centre = [(i - 1) / 2.0 for i in shape]
    out = torch.empty((3,) + shape, dtype=torch.float32, device=dev)
    lat = torch.from_numpy(np.ascontiguousarray(plan.lattice, dtype=np.float32)).to(dev) if plan.lattice is not None else None
    sh = torch.from_numpy(np.ascontiguousarray(plan.shifts, dtype=np.int32)).to(dev) if plan.shifts is not None else None
    if sh is not None and tuple(sh.shape) != (2, shape[0]):
        raise ValueError(f"shifts of shape {tuple(sh.shape)} for {shape[0]} sections")
    mirror = sum(1 << a for a in range(3) if plan.mirror[a])
    _lib.check(_lib.lib.bsmi_aug_coords(
        dev.index, _lib.i64x3(shape), _f32(plan.linear), _f32(centre), _f32([c - lo for c, lo in zip(centre, box_lo)]), mirror,
        1 if plan.swap else 0, C.c_void_p(sh.data_ptr()) if sh is not None else None, C.c_void_p(lat.data_ptr()) if lat is not None else None,
        (C.c_int32 * 3)(*lat.shape[1:]) if lat is not None else None, _f32(plan.inv_spacing) if lat is not None else None,
        C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    for t in (lat, sh):   # uploaded on this stream, read by the launch queued on it
        if t is not None:
            t.record_stream(torch.cuda.current_stream(dev))
    return out


def _sample(fn, coords_dev, crop, region, crop_dtype, out_dtype):
    import torch
    from . import _lib
    if coords_dev.dtype != torch.float32 or coords_dev.dim() != 4 or coords_dev.shape[0] != 3 or not coords_dev.is_cuda or not coords_dev.is_contiguous():
        raise ValueError("coords must be a contiguous float32 CUDA tensor (3, D, H, W)")
    if crop.dtype != crop_dtype or crop.dim() != 3 or crop.device != coords_dev.device or not crop.is_contiguous():
        raise ValueError(f"crop must be a contiguous {crop_dtype} tensor (D, H, W) on the coordinates' device")
    off, shape = ((0, 0, 0), tuple(coords_dev.shape[1:])) if region is None else (tuple(int(v) for v in region[0]), tuple(int(v) for v in region[1]))
    out = torch.empty(shape, dtype=out_dtype, device=crop.device)
    _lib.check(getattr(_lib.lib, fn)(
        crop.device.index, C.c_void_p(coords_dev.data_ptr()), _lib.i64x3(coords_dev.shape[1:]), _lib.i64x3(off), _lib.i64x3(shape),
        C.c_void_p(crop.data_ptr()), _lib.i64x3(crop.shape), C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(crop.device).cuda_stream)))
    return out


def sample_raw(coords_dev, crop, region=None):
    """uint8 crop -> float32 `region` ((offset, shape) inside the coordinate volume; default all of it): trilinear, v * 2 / 255 - 1"""
    import torch
    return _sample("bsmi_aug_sample_f32_u8", coords_dev, crop, region, torch.uint8, torch.float32)


def sample_labels(coords_dev, crop, region=None):
    """int64 crop -> int64 region: nearest, floor(s + 1/2) per axis in float32"""
    import torch
    return _sample("bsmi_aug_sample_nearest_i64", coords_dev, crop, region, torch.int64, torch.int64)


def sample_mask(coords_dev, crop, region=None):
    """uint8 crop -> uint8 region: nearest, as the labels"""
    import torch
    return _sample("bsmi_aug_sample_nearest_u8", coords_dev, crop, region, torch.uint8, torch.uint8)
