"""Geometric training augmentation of the 2-D setups on the device: SimpleAugment -> DeformAugment -> ShiftAugment of
2d_affs, 2d_lsd and 2d_mtlsd (reference models/2d_mtlsd/train.py:112-122 and its siblings), under gp.Stack(10): a step is S
independent draws of one output section each, every draw with its own plan.  The chain is composed into ONE coordinate map
per draw and applied to the whole batch by the launches of csrc/augment2d.hip: bsmi_aug2d_coords writes the source
coordinate of every pixel of every draw's frame, for all K = adj_slices sections of raw; bsmi_aug2d_sample_* resample raw
(bilinear), labels and mask (nearest) of all draws through them, one launch per array.

These are specified rules (restated in float64 by tests/aug2d_ref.py), not a transcription of
gunpowder, which is not installed where this was written: parity with the reference is in distribution, not draw by draw.
With I = (H, W) the input section, O the output section, ctx = (I - O) / 2, c = (I - 1) / 2, k a section of the raw stack
(the labels' section is K // 2) and (y, x) a pixel in the input section's own frame, which may lie outside [0, I):

    r      = (y + sh_y[k], x + sh_x[k])      ShiftAugment: integer shift of section k (drawn only when K > 1)
    t      = A (r - c) + E(r)                DeformAugment(spatial_dims=2): A = u R(theta), E = bilinear elastic displacement
    s      = c_src + M t                     SimpleAugment: y <-> x swap, then the y and x mirrors; c_src = c in the crop's pixels
    k_src  = K - 1 - k if the z mirror is set, else k: z is never interpolated

The map is evaluated over a FRAME, the union of the input section and the labels window grown by the targets' context
(per axis F_lo = min(0, ctx - lo), F_hi = max(I, ctx + O + hi), lo / hi SectionSource's label margins): the shipped 2d_mtlsd
net needs 60 pixels of labels beyond its output section at a 4 nm grid against a network context of 46.  The lattice spans
the frame: node j at F_lo + (j - 1) spacing, j = 0 .. ceil((F_hi - F_lo - 1) / spacing) + 2.

Declared differences, as for the 3-D chain (augment.py): E is evaluated at every pixel (the reference's subsample=4 is a CPU
shortcut); the 5 % rejection test sees the augmented output window, and it is per slot of the batch.  ShiftAugment's
probability `shift_p` defaults to 1.0: the 2-D call sites pass no `p`, and 1.0 is gunpowder's documented default.

With `intensity` inside the table, raw then runs through the reference's intensity nodes (models/2d_mtlsd/train.py:123-136 and
its siblings: NoiseAugment -> IntensityAugment -> GammaAugment -> ImpulseNoiseAugment -> SmoothAugment -> DefectAugment), again
one launch per node for the WHOLE batch (csrc/augment2d_intensity.hip), driven by a table of per-draw descriptors and per-plane
tables (PackedIntensity2D, apply_intensity2d).  The rule for a draw is augment.py's rule for the block (K, H, W) of its K
sections, unchanged and the same device code, so the results are the same bits (DESIGN.md sections 7k and 7m): the Philox
counter is the voxel's index inside the draw's own stack, smoothing runs over all three axes of the stack with the draw's
sigma.  The call-site defaults that differ from the 3-D setups: prob_missing is 0.05 when adj_slices > 1 and 0 when it is 1
(models/2d_mtlsd/train.py:136), resolved where adj_slices is known (Aug2DParams.intensity_for).
NOT built: the deformation and artifact sources of DefectAugment, ClaheAugment, augmentation of SyntheticSource.
"""
import ctypes as C
import dataclasses
import math

import numpy as np

from .augment import IntensityParams, _interval_mul

# what the trainer's log line names as missing
NOT_BUILT = "the deformation and artifact sources of DefectAugment, and ClaheAugment"
INTENSITY_NODES = "NoiseAugment, IntensityAugment, GammaAugment, ImpulseNoiseAugment, SmoothAugment and DefectAugment of raw"
MAX_LATTICE_NODES = 4096   # csrc/augment2d.hip: 32 KiB of offsets in LDS per draw


@dataclasses.dataclass(frozen=True)
class Aug2DParams:
    """The arguments of the three nodes; the defaults are the reference's (models/2d_mtlsd/train.py:112-122).
    control_point_spacing / jitter_sigma: two world-unit values (y, x), None = the reference's (vs_y vs_z, vs_x vs_z) and
    (2 vs_y, 2 vs_x).  shift_p: 1.0, gunpowder's documented default (the 2-D call passes none).  intensity: an
    augment.IntensityParams turns on the intensity chain of raw; None (the default, also of `augment2d = true`): the geometric
    chain alone.  Its prob_missing is None where the config gives none: the reference's default depends on adj_slices, so
    intensity_for(K) resolves it."""
    simple: bool = True
    deform_p: float = 0.5
    scale_interval: tuple = (0.9, 1.1)
    rotate: bool = True
    control_point_spacing: tuple = None
    jitter_sigma: tuple = None
    shift_p: float = 1.0
    prob_slip: float = 0.2
    prob_shift: float = 0.2
    shift_sigma: float = 3.0
    intensity: IntensityParams = None

    def intensity_for(self, sections):
        """the IntensityParams of a setup with K = `sections`: prob_missing, where the config gives none, is the reference's 0.05
        for K > 1 and 0 for K = 1 (models/2d_mtlsd/train.py:136); None without the key"""
        if self.intensity is None or self.intensity.prob_missing is not None:
            return self.intensity
        return dataclasses.replace(self.intensity, prob_missing=0.05 if int(sections) > 1 else 0.0)

    @classmethod
    def from_config(cls, value):
        """The train TOML key `augment2d`: absent / false -> None (today's path), true -> the defaults, a table -> overrides."""
        if value is None or value is False:
            return None
        if value is True:
            return cls()
        if not isinstance(value, dict):
            raise ValueError(f"augment2d must be true, false or a table, not {value!r}")
        names = [f.name for f in dataclasses.fields(cls)]
        unknown = sorted(set(value) - set(names))
        if unknown:
            raise ValueError(f"unknown augment2d key(s) {', '.join(unknown)}; known: {', '.join(names)}")
        kw = {}
        for k, v in value.items():
            if k == "intensity":
                # augment.IntensityParams' keys, checks and error texts.  Without prob_missing the table is checked with 0.05, the
                # larger of the two defaults, and the field is left open for intensity_for
                if v is True or (isinstance(v, dict) and "prob_missing" not in v):
                    checked = IntensityParams.from_config(dict({} if v is True else v, prob_missing=0.05), "augment2d.intensity")
                    kw[k] = dataclasses.replace(checked, prob_missing=None)
                else:
                    kw[k] = IntensityParams.from_config(v, "augment2d.intensity")
            elif k in ("simple", "rotate"):
                kw[k] = bool(v)
            elif k == "scale_interval":
                kw[k] = tuple(float(x) for x in v)
                if len(kw[k]) != 2 or not 0 < kw[k][0] <= kw[k][1]:
                    raise ValueError(f"augment2d.scale_interval {v!r}: two positive numbers, low <= high")
            elif k in ("control_point_spacing", "jitter_sigma"):
                kw[k] = tuple(float(x) for x in v)
                if len(kw[k]) != 2 or (k == "control_point_spacing" and min(kw[k]) <= 0) or min(kw[k]) < 0:
                    raise ValueError(f"augment2d.{k} {v!r}: two world-unit values (y, x)")
            else:
                kw[k] = float(v)
                if kw[k] < 0 or (k != "shift_sigma" and kw[k] > 1):
                    raise ValueError(f"augment2d.{k} {v!r}: " + ("not negative" if k == "shift_sigma" else "a probability"))
        return cls(**kw)


@dataclasses.dataclass
class Aug2DPlan:
    """One draw's plan, held in the number formats the kernel reads (float32 / int32), so that the float64 restatement
    starts from the same numbers.  shape: I = (H, W).  frame: ((F_lo_y, F_lo_x), (F_hi_y, F_hi_x)) in the input section's
    pixels, hi exclusive.  sections: K.  mirror: 3 flags (z, y, x).  swap: y <-> x.  u, theta: what was drawn; linear:
    float32 [4] = u * (cos, -sin, sin, cos), row-major A.  lattice: float32 [2, n_y, n_x] control offsets in pixels
    (component y, x) or None; inv_spacing: float32 [2], 1 / (node spacing in pixels).  shifts: int32 [2, K] (y, x per
    section) or None."""
    shape: tuple
    frame: tuple = None
    sections: int = 1
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
        if self.frame is None:
            self.frame = ((0, 0), self.shape)
        self.frame = (tuple(int(v) for v in self.frame[0]), tuple(int(v) for v in self.frame[1]))
        self.sections = int(self.sections)
        if self.linear is None:
            self.linear = linear_of(self.u, self.theta)

    @property
    def frame_shape(self):
        return tuple(h - l for l, h in zip(*self.frame))


def linear_of(u, theta):
    """float32 (a0 .. a3) = u * (cos, -sin, sin, cos): t_y = a0 d_y + a1 d_x, t_x = a2 d_y + a3 d_x"""
    c, s = math.cos(theta), math.sin(theta)
    return np.array([u * c, -u * s, u * s, u * c], dtype=np.float32)


def frame_of(inp, out, lo, hi):
    """The frame of a draw: per axis F_lo = min(0, ctx - lo), F_hi = max(I, ctx + O + hi) -- the union of the input section
    and the output window grown by the label margins lo / hi.  -> ((F_lo_y, F_lo_x), (F_hi_y, F_hi_x))"""
    ctx = [(i - o) // 2 for i, o in zip(inp, out)]
    return (tuple(min(0, c - l) for c, l in zip(ctx, lo)), tuple(max(i, c + o + h) for i, c, o, h in zip(inp, ctx, out, hi)))


def lattice_shape(frame, spacing):
    """Nodes per axis of a lattice with `spacing` pixels between nodes over the frame: node j at F_lo + (j - 1) * spacing,
    j = 0 .. ceil((F_hi - F_lo - 1) / spacing) + 2 (the frame plus one node on each side)"""
    return tuple(int(math.ceil((h - l - 1) / sp)) + 3 for l, h, sp in zip(frame[0], frame[1], spacing))


def check_square(inp, out):
    if inp[0] != inp[1] or out[0] != out[1]:
        raise ValueError(f"the y/x swap of SimpleAugment needs square sections, not input {list(inp)} / output {list(out)}; "
                         "set augment2d.simple = false")


def check_rotation(voxel_size):
    if float(voxel_size[1]) != float(voxel_size[2]):
        raise NotImplementedError(f"rotation in the section plane needs voxel_size[1] == voxel_size[2], not {list(voxel_size)}; "
                                  "set augment2d.rotate = false")


def draw_plan2d(rng, params, shape, frame, sections, voxel_size):
    """One plan for an input section of `shape` = (H, W) with `frame` and K = `sections`, every draw taken from `rng` (a numpy
    Generator: the sample source's own stream) in this order; a node whose probability is 0 or that is switched off takes no
    draw at all.
      1. simple:  4 x rng.random() < 0.5 -- mirror z, mirror y, mirror x, swap y/x
      2. deform:  rng.random() < deform_p; if applied: u = rng.uniform(*scale_interval); theta = rng.uniform(0, 2 pi)
                  (only when rotate); the lattice, rng.standard_normal((2, n_y, n_x)) * sigma (pixels) per component
      3. shift:   only when K > 1: rng.random() < shift_p; if applied: rng.random(K) < prob_shift,
                  rint(rng.normal(0, sigma, (K, 2))) -- added to this section and all later ones; rng.random(K) < prob_slip,
                  rint(rng.normal(0, sigma, (K, 2))) -- added to this section alone.
    voxel_size: (z, y, x) world units."""
    shape = tuple(int(v) for v in shape)
    vs = [float(v) for v in voxel_size]
    k = int(sections)
    plan = Aug2DPlan(shape, frame, k)
    if params.simple:
        if shape[0] != shape[1]:
            check_square(shape, shape)
        flags = [bool(rng.random() < 0.5) for _ in range(4)]
        plan.mirror, plan.swap = tuple(flags[:3]), flags[3]
    if params.deform_p > 0 and rng.random() < params.deform_p:
        if params.rotate:
            check_rotation(vs)
        plan.u = float(rng.uniform(*params.scale_interval))
        plan.theta = float(rng.uniform(0.0, 2.0 * math.pi)) if params.rotate else 0.0
        plan.linear = linear_of(plan.u, plan.theta)
        cps = params.control_point_spacing or (vs[1] * vs[0], vs[2] * vs[0])
        sig = params.jitter_sigma or (2.0 * vs[1], 2.0 * vs[2])
        spacing = [c / v for c, v in zip(cps, vs[1:])]
        n = lattice_shape(plan.frame, spacing)
        if n[0] * n[1] > MAX_LATTICE_NODES:
            raise ValueError(f"control lattice of {n} nodes for a frame of {list(plan.frame_shape)} at spacing {spacing} pixels: at most "
                             f"{MAX_LATTICE_NODES}")
        sv = np.array([s / v for s, v in zip(sig, vs[1:])]).reshape(2, 1, 1)
        plan.lattice = (rng.standard_normal((2,) + n) * sv).astype(np.float32)
        plan.inv_spacing = np.array([1.0 / sp for sp in spacing], dtype=np.float32)
    if k > 1 and params.shift_p > 0 and rng.random() < params.shift_p:
        on = rng.random(k) < params.prob_shift
        step = np.rint(rng.normal(0.0, params.shift_sigma, (k, 2)))
        slip_on = rng.random(k) < params.prob_slip
        slip = np.rint(rng.normal(0.0, params.shift_sigma, (k, 2)))
        total = np.cumsum(step * on[:, None], axis=0) + slip * slip_on[:, None]
        plan.shifts = np.ascontiguousarray(total.T).astype(np.int32)
    return plan


def source_box2d(plan, region=None):
    """(lo, hi): an integer box, in pixels relative to the input section's origin, hi exclusive, that contains s -- taken with
    c_src = c -- and its bilinear neighbour floor(s) + 1 for every pixel of `region` ((offset, shape) in the input section's
    pixels; default: the whole frame) and every section.  The crop read for a draw is this box, so c_src = c - lo.

    The bound, by the interval arithmetic of augment.source_box.  Per axis, r_a - c_a lies in [o_a - c_a + min sh_a, o_a + n_a -
    1 - c_a + max sh_a] (the shifts of all K sections).  A (r - c) is linear, so each component lies in the sum of the
    intervals a_k * [lo, hi] of its terms.  E(r) is a bilinear, i.e. convex, combination of lattice offsets (the lattice
    coordinate is clamped to the lattice), so |E_a| <= max |lattice[a]|.  The swap exchanges the two intervals, a mirror
    negates one.  That bounds the exact map; the kernel's float32 result differs from it by far less than a pixel
    (tests/aug2d_ref.py: coords_gate), so one pixel of margin below and, with the neighbour floor(s) + 1, two above make
    the box safe.  It is conservative."""
    shape = plan.shape
    off, n = (plan.frame[0], plan.frame_shape) if region is None else (tuple(region[0]), tuple(region[1]))
    lin = [float(v) for v in plan.linear]
    d = []
    for a in range(2):
        c = (shape[a] - 1) / 2.0
        s_lo = s_hi = 0
        if plan.shifts is not None:
            s_lo, s_hi = int(plan.shifts[a].min()), int(plan.shifts[a].max())
        d.append((off[a] - c + s_lo, off[a] + n[a] - 1 - c + s_hi))
    emax = [float(np.abs(plan.lattice[a]).max()) for a in range(2)] if plan.lattice is not None else [0.0, 0.0]

    def add(*ivs):
        return sum(i[0] for i in ivs), sum(i[1] for i in ivs)
    t = [add(_interval_mul(lin[0], *d[0]), _interval_mul(lin[1], *d[1]), (-emax[0], emax[0])),
         add(_interval_mul(lin[2], *d[0]), _interval_mul(lin[3], *d[1]), (-emax[1], emax[1]))]
    if plan.swap:
        t = [t[1], t[0]]
    lo, hi = [], []
    for a in range(2):
        a_lo, a_hi = (-t[a][1], -t[a][0]) if plan.mirror[a + 1] else t[a]
        c = (shape[a] - 1) / 2.0
        lo.append(int(math.floor(c + a_lo)) - 1)
        hi.append(int(math.ceil(c + a_hi)) + 3)
    return tuple(lo), tuple(hi)


class Packed2D:
    """The S plans of one batch (or of the slots of a batch that are drawn again) in the form the launches read: the table of
    per-draw descriptors (bsmi_aug2d_draw of include/bsmi.h), the lattices of all draws packed into one float32 buffer, the
    shifts as int32 [S][2][K] (None when no draw has any) and, per draw, the crop's shape and its pixel offset in the packed
    crops.  boxes: source_box2d of each plan, (lo, hi); crops differ in shape from draw to draw.  Host memory only; coords2d
    uploads it, once, for the four launches."""

    def __init__(self, plans, boxes):
        from . import _lib
        if not plans or len(plans) != len(boxes):
            raise ValueError("one box per plan, at least one plan")
        p0 = plans[0]
        if any(p.shape != p0.shape or p.frame != p0.frame or p.sections != p0.sections for p in plans):
            raise ValueError("the plans of a batch share the input section, the frame and the number of sections")
        self.S, self.K, self.shape, self.frame = len(plans), p0.sections, p0.shape, p0.frame
        self.frame_shape = p0.frame_shape
        self.draws = (_lib.Aug2dDraw * self.S)()
        self.crop_shapes, self.crop_offsets = [], []
        lattices, lat_off, crop_off = [], 0, 0
        shifts = np.zeros((self.S, 2, self.K), dtype=np.int32)
        for s, (plan, (lo, hi)) in enumerate(zip(plans, boxes)):
            d = self.draws[s]
            d.a[:] = [float(v) for v in plan.linear]
            d.src[:] = [(i - 1) / 2.0 - l for i, l in zip(plan.shape, lo)]
            d.flags = sum(1 << a for a in range(3) if plan.mirror[a]) | (8 if plan.swap else 0)
            if plan.lattice is not None:
                lat = np.ascontiguousarray(plan.lattice, dtype=np.float32)
                if lat.ndim != 3 or lat.shape[0] != 2:
                    raise ValueError(f"lattice of shape {lat.shape}: (2, n_y, n_x)")
                d.n[:] = lat.shape[1:]
                d.inv_spacing[:] = [float(v) for v in plan.inv_spacing]
                d.lattice_offset = lat_off
                lattices.append(lat.ravel())
                lat_off += lat.size
            if plan.shifts is not None:
                if tuple(plan.shifts.shape) != (2, self.K):
                    raise ValueError(f"shifts of shape {tuple(plan.shifts.shape)} for {self.K} sections")
                shifts[s] = plan.shifts
            crop = tuple(int(h - l) for l, h in zip(lo, hi))
            d.crop[:] = crop
            d.crop_offset = crop_off
            self.crop_shapes.append(crop)
            self.crop_offsets.append(crop_off)
            crop_off += crop[0] * crop[1]
        self.crop_pixels = crop_off
        self.lattice = np.concatenate(lattices) if lattices else None
        self.shifts = shifts if any(p.shifts is not None for p in plans) else None
        self.dev = None   # device copies: (draws, lattice, shifts), made by coords2d

    def pack(self, crops, dtype):
        """the draws' crops -- (crop_h, crop_w) each, or (K, crop_h, crop_w) for raw -- as one 1-D array in draw order"""
        for s, c in enumerate(crops):
            if tuple(c.shape[-2:]) != self.crop_shapes[s] or c.ndim not in (2, 3) or (c.ndim == 3 and c.shape[0] != self.K):
                raise ValueError(f"crop {s} of shape {tuple(c.shape)} for a box of {self.crop_shapes[s]} ({self.K} sections of raw)")
        return np.concatenate([np.ascontiguousarray(c, dtype=dtype).ravel() for c in crops])


# ---- device wrappers (libbsmi: include/bsmi.h, "training augmentation of the 2-D setups") ----

def _i64x2(v):
    return (C.c_int64 * 2)(*[int(x) for x in v])


def coords2d(packed, device=0):
    """The source coordinates of every draw, section and frame pixel, in pixels of each draw's crop: float32 CUDA
    (S, K, 2, F_h, F_w).  Uploads the descriptor table, the packed lattices and the shifts (kept in packed.dev)."""
    import torch
    from . import _lib
    dev = torch.device("cuda", device) if not isinstance(device, torch.device) else device
    stream = torch.cuda.current_stream(dev)
    table = torch.from_numpy(np.frombuffer(packed.draws, dtype=np.uint8).copy()).to(dev)
    lat = torch.from_numpy(packed.lattice).to(dev) if packed.lattice is not None else None
    sh = torch.from_numpy(packed.shifts).to(dev) if packed.shifts is not None else None
    packed.dev = (table, lat, sh)
    out = torch.empty((packed.S, packed.K, 2) + packed.frame_shape, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib.bsmi_aug2d_coords(
        dev.index, packed.draws, C.c_void_p(table.data_ptr()), packed.S, packed.K, _i64x2(packed.shape), _i64x2(packed.frame[0]),
        _i64x2(packed.frame_shape), C.c_void_p(sh.data_ptr()) if sh is not None else None, C.c_void_p(lat.data_ptr()) if lat is not None else None,
        int(lat.numel()) if lat is not None else 0, C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream)))
    for t in packed.dev:   # uploaded on this stream, read by the launches queued on it
        if t is not None:
            t.record_stream(stream)
    return out


def _sample(fn, packed, coords_dev, crops, region, crop_dtype, out_dtype, sections, ipacked=None):
    import torch
    from . import _lib
    want = (packed.S, packed.K, 2) + packed.frame_shape
    if coords_dev.dtype != torch.float32 or tuple(coords_dev.shape) != want or not coords_dev.is_cuda or not coords_dev.is_contiguous():
        raise ValueError(f"coords must be coords2d of this batch: a contiguous float32 CUDA tensor {want}")
    if packed.dev is None or packed.dev[0].device != coords_dev.device:
        raise ValueError("the descriptor table is not on the coordinates' device (coords2d uploads it)")
    if crops.dtype != crop_dtype or crops.dim() != 1 or crops.device != coords_dev.device or not crops.is_contiguous():
        raise ValueError(f"crops must be a contiguous 1-D {crop_dtype} tensor (Packed2D.pack) on the coordinates' device")
    if crops.numel() != packed.crop_pixels * sections:
        raise ValueError(f"packed crops of {crops.numel()} pixels, not {packed.crop_pixels} x {sections}")
    lo = packed.frame[0]
    off, shape = (lo, packed.frame_shape) if region is None else (tuple(int(v) for v in region[0]), tuple(int(v) for v in region[1]))
    lead = (packed.K, packed.S) if crop_dtype == torch.uint8 and out_dtype == torch.float32 else (packed.S,)   # raw: the trainer's layout
    out = torch.empty(lead + shape, dtype=out_dtype, device=crops.device)
    itable = () if ipacked is None else (ipacked.idraws, C.c_void_p(ipacked.upload(crops.device)[0].data_ptr()))
    _lib.check(getattr(_lib.lib, fn)(
        crops.device.index, packed.draws, C.c_void_p(packed.dev[0].data_ptr()), *itable, packed.S, packed.K, C.c_void_p(coords_dev.data_ptr()),
        _i64x2(packed.frame_shape), _i64x2([o - l for o, l in zip(off, lo)]), _i64x2(shape), C.c_void_p(crops.data_ptr()), int(crops.numel()),
        C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(crops.device).cuda_stream)))
    return out


def sample_raw2d(packed, coords_dev, crops, region=None):
    """packed uint8 crops (K sections per draw) -> float32 (K, S, h, w) over `region` ((offset, shape) in the input section's
    pixels; default the whole frame): bilinear in the plane of section k_src, v * 2 / 255 - 1"""
    import torch
    return _sample("bsmi_aug2d_sample_f32_u8", packed, coords_dev, crops, region, torch.uint8, torch.float32, packed.K)


def sample_labels2d(packed, coords_dev, crops, region=None):
    """packed int64 crops (one section per draw) -> int64 (S, h, w): nearest, floor(s + 1/2) per axis in float32, through the
    coordinates of section K // 2"""
    import torch
    return _sample("bsmi_aug2d_sample_nearest_i64", packed, coords_dev, crops, region, torch.int64, torch.int64, 1)


def sample_mask2d(packed, coords_dev, crops, region=None):
    """packed uint8 crops (one section per draw) -> uint8 (S, h, w): nearest, as the labels"""
    import torch
    return _sample("bsmi_aug2d_sample_nearest_u8", packed, coords_dev, crops, region, torch.uint8, torch.uint8, 1)


# ---- the intensity chain of the whole batch (include/bsmi.h, "training augmentation of the 2-D setups: the intensity chain") ----

NOISE, INTENSITY, GAMMA, IMPULSE, SMOOTH, DEFECT, TOUCHED = 1, 2, 4, 8, 16, 32, 64   # BSMI_AUG2D_*: the bits of a descriptor's `nodes`


def node_bits(plan):
    """the descriptor bits of an augment.IntensityPlan; TOUCHED = plan.applied"""
    bits = ((NOISE if plan.noise_sigma is not None else 0) | (INTENSITY if plan.scale is not None else 0) | (GAMMA if plan.gamma is not None else 0)
            | (IMPULSE if plan.impulse_threshold is not None else 0) | (SMOOTH if plan.weights is not None else 0)
            | (DEFECT if plan.defect is not None else 0))
    return bits | (TOUCHED if plan.applied else 0)


class PackedIntensity2D:
    """The S intensity plans of one batch (augment.IntensityPlan, each for a stack (K, H, W); a draw that is not to be touched
    holds a plan without an applied node) in the form the launches read: the table of per-draw descriptors (bsmi_aug2d_idraw of
    include/bsmi.h: node bits, seed, noise sigma, impulse threshold, contrast scale, smoothing radius and the offset of its taps),
    the per-plane tables -- plane p = k * S + s of the trainer's layout [K][S][H][W] -- as ONE array `planes` [4][K * S] of 32-bit
    words (rows: scale, shift, gamma exponent as float32; defect mode as int32; rows of draws without the node hold 1, 0, 1, 0)
    and the taps of all smoothed draws packed into one float32 buffer.  Host memory; upload() makes the device copies, at most
    three small uploads."""

    def __init__(self, plans):
        from . import _lib
        if not plans:
            raise ValueError("at least one plan")
        shape = tuple(int(v) for v in plans[0].shape)
        if len(shape) != 3 or any(tuple(p.shape) != shape for p in plans):
            raise ValueError("the plans of a batch share one stack shape (K, H, W)")
        self.S, self.K, self.section = len(plans), shape[0], shape[1:]
        S, K = self.S, self.K
        self.idraws = (_lib.Aug2dIDraw * S)()
        self.planes = np.zeros((4, K * S), dtype=np.int32)
        fl = self.planes.view(np.float32)
        fl[0], fl[2] = 1.0, 1.0
        taps, off = [], 0
        self.nodes = 0
        for s, plan in enumerate(plans):
            d = self.idraws[s]
            d.nodes = node_bits(plan)
            self.nodes |= d.nodes
            d.seed = int(plan.seed)
            d.noise_sigma = float(plan.noise_sigma) if plan.noise_sigma is not None else 0.0
            d.impulse_threshold = int(plan.impulse_threshold) if plan.impulse_threshold is not None else 0
            d.contrast_scale = float(plan.contrast_scale)
            for row, values in ((0, plan.scale), (1, plan.shift), (2, plan.gamma)):
                if values is not None:
                    fl[row, s::S] = self._per_section(values, np.float32, K)
            if plan.defect is not None:
                self.planes[3, s::S] = self._per_section(plan.defect, np.int32, K)
            if plan.weights is not None:
                w = np.ascontiguousarray(plan.weights, dtype=np.float32)
                if w.ndim != 1 or w.size % 2 != 1:
                    raise ValueError("weights: 2 radius + 1 taps")
                d.radius, d.taps_offset = w.size // 2, off
                taps.append(w)
                off += w.size
        self.taps = np.concatenate(taps) if taps else None
        self.low_contrast = bool(((self.planes[3] == 3)).any())
        self.dev = None   # device copies: (idraws, planes, taps)

    @staticmethod
    def _per_section(values, dtype, K):
        v = np.asarray(values)
        if v.dtype != dtype or v.shape != (K,):
            raise ValueError(f"one {np.dtype(dtype)} value per section ({K}), not {v.dtype} {v.shape}")
        return v

    @property
    def touched(self):
        """per draw, whether the chain changes it (its plan's `applied`)"""
        return [bool(d.nodes & TOUCHED) for d in self.idraws]

    def upload(self, device=0):
        """the device copies, once: the descriptor table, the per-plane tables, the taps (only where a draw is smoothed)"""
        import torch
        dev = torch.device("cuda", device) if not isinstance(device, torch.device) else device
        if self.dev is None or self.dev[0].device != dev:
            stream = torch.cuda.current_stream(dev)
            table = torch.from_numpy(np.frombuffer(self.idraws, dtype=np.uint8).copy()).to(dev)
            planes = torch.from_numpy(self.planes).to(dev)
            taps = torch.from_numpy(self.taps).to(dev) if self.taps is not None else None
            self.dev = (table, planes, taps)
            for t in self.dev:   # uploaded on this stream, read by the launches queued on it
                if t is not None:
                    t.record_stream(stream)
        return self.dev


def sample_unit2d(packed, coords_dev, crops, ipacked, region=None):
    """sample_raw2d for a batch that goes on through the intensity chain: the draws `ipacked` (a PackedIntensity2D of the same S
    draws) marks as touched are written v / 255, what the chain starts from; the others v * 2 / 255 - 1, bit-equal to sample_raw2d"""
    import torch
    if ipacked.S != packed.S or ipacked.K != packed.K:
        raise ValueError(f"intensity table of {ipacked.S} draws x {ipacked.K} sections for a batch of {packed.S} x {packed.K}")
    return _sample("bsmi_aug2d_sample_unit_f32_u8", packed, coords_dev, crops, region, torch.uint8, torch.float32, packed.K, ipacked)


def _batch(x, ipacked):
    """the leading arguments of a batched node: device, the table twice, S, K, the section's shape, the batch"""
    import torch
    want = (ipacked.K, ipacked.S) + tuple(ipacked.section)
    if x.dtype != torch.float32 or tuple(x.shape) != want or not x.is_cuda or not x.is_contiguous():
        raise ValueError(f"the batch must be a contiguous float32 CUDA tensor {want}")
    table = ipacked.upload(x.device)[0]
    return (x.device.index, ipacked.idraws, C.c_void_p(table.data_ptr()), ipacked.S, ipacked.K, _i64x2(ipacked.section), C.c_void_p(x.data_ptr()))


def _stream(x):
    import torch
    return C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)


def _row(ipacked, x, row):
    planes = ipacked.upload(x.device)[1]
    return C.c_void_p(planes[row].data_ptr())


def plane_stats(x):
    """float32 CUDA (K * S, 3): mean, min and max of every plane of the batch (K, S, H, W), in augment.section_stats' fixed order"""
    from .augment import section_stats
    return section_stats(x.view((x.shape[0] * x.shape[1],) + tuple(x.shape[2:])))


def _stats(x, stats):
    import torch
    if stats.dtype != torch.float32 or tuple(stats.shape) != (x.shape[0] * x.shape[1], 3) or stats.device != x.device or not stats.is_contiguous():
        raise ValueError("stats must be plane_stats of the batch: float32 (K * S, 3) on its device")
    return C.c_void_p(stats.data_ptr())


def noise2d(x, ipacked):
    """NoiseAugment of every draw that has it, one launch; x (K, S, H, W) in place"""
    from . import _lib
    _lib.check(_lib.lib.bsmi_aug2d_noise_f32(*_batch(x, ipacked), _stream(x)))
    return x


def impulse2d(x, ipacked):
    from . import _lib
    _lib.check(_lib.lib.bsmi_aug2d_impulse_f32(*_batch(x, ipacked), _stream(x)))
    return x


def intensity2d(x, ipacked, stats):
    from . import _lib
    _lib.check(_lib.lib.bsmi_aug2d_intensity_f32(*_batch(x, ipacked), _stats(x, stats), _row(ipacked, x, 0), _row(ipacked, x, 1), _stream(x)))
    return x


def gamma2d(x, ipacked, stats):
    from . import _lib
    _lib.check(_lib.lib.bsmi_aug2d_gamma_f32(*_batch(x, ipacked), _stats(x, stats), _row(ipacked, x, 2), _stream(x)))
    return x


def smooth2d(x, ipacked, tmp=None):
    """SmoothAugment of every draw that has it, each with its own taps over its own K sections: two launches"""
    import torch
    from . import _lib
    if ipacked.taps is None:
        return x
    tmp = torch.empty_like(x) if tmp is None else tmp
    taps = ipacked.upload(x.device)[2]
    _lib.check(_lib.lib.bsmi_aug2d_smooth_f32(*_batch(x, ipacked), C.c_void_p(tmp.data_ptr()), C.c_void_p(taps.data_ptr()), int(taps.numel()),
                                              _stream(x)))
    return x


def defect2d(x, ipacked, stats=None, final_map=False):
    """DefectAugment of every draw that has it (stats: plane_stats, needed where a section is low-contrast); final_map: then
    2 x - 1 on every touched draw"""
    from . import _lib
    modes = ipacked.planes[3]
    _lib.check(_lib.lib.bsmi_aug2d_defect_f32(*_batch(x, ipacked), _stats(x, stats) if stats is not None else None,
                                              modes.ctypes.data_as(C.POINTER(C.c_int32)), _row(ipacked, x, 3), 1 if final_map else 0, _stream(x)))
    return x


def apply_intensity2d(raw_t, packed, final_map=True):
    """The intensity chain of the whole batch raw_t (K, S, H, W) -- touched draws in [0, 1], as sample_unit2d writes them -- in
    place: one launch per node that some draw applies (smooth: two), the plane statistics its successor needs, then 2 x - 1 on
    the touched draws.  At most 13 launches whatever S is; a batch without a touched draw launches nothing.  Draw s comes out as
    augment.apply_intensity leaves the stack raw_t[:, s] under its plan, bit for bit; an untouched draw stays bit-equal."""
    n = packed.nodes
    if not n & TOUCHED:
        return raw_t
    if n & NOISE:
        noise2d(raw_t, packed)
    if n & INTENSITY:
        intensity2d(raw_t, packed, plane_stats(raw_t))
    if n & GAMMA:
        gamma2d(raw_t, packed, plane_stats(raw_t))
    if n & IMPULSE:
        impulse2d(raw_t, packed)
    if n & SMOOTH:
        smooth2d(raw_t, packed)
    return defect2d(raw_t, packed, plane_stats(raw_t) if packed.low_contrast else None, final_map)
