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

With `intensity` inside the table, raw then runs through the reference's intensity nodes (models/3d_mtlsd/train.py:117-132
and its siblings) on the device, one launch of csrc/augment_intensity.hip per node, in the reference's order: NoiseAugment
-> IntensityAugment -> GammaAugment -> ImpulseNoiseAugment -> SmoothAugment -> DefectAugment.  These too are specified rules
(restated in float64 by tests/intensity_ref.py): gunpowder and skimage are not installed where this
was written, so parity is in distribution.  x is raw in [0, 1], sections are the z planes:

    resample   the trilinear expression above, written v / 255
    noise      x = clip(x + sqrt(noise_var) n), n a standard normal per voxel (Philox4x32-10 on the device)
    intensity  x = clip(m_z + (x - m_z) scale_z + shift_z), m_z the section's mean
    gamma      x = ((x - a) / (b - a))^g_z (b - a) + a with a, b the section's extrema, where b - a > 1e-3
    impulse    a voxel is replaced with probability q by a value in U[0, 1)
    smooth     scipy.ndimage.gaussian_filter(x, sigma) over all three axes: radius int(4 sigma + 0.5), border reflect
    defect     per section: 0 or 1 throughout (prob_missing), or x = m + (x - m) contrast_scale (prob_low_contrast)
    output     2 x - 1

Declared quirk: the reference's ImpulseNoiseAugment draws its locations with the node's p, not with the pixel_p its call
site passes (gp/impulse_noise_augment.py:58), so the default of `impulse_pixel_p` is q = impulse_p, what the reference
executes; setting the key gives the documented 0.05 or any other value.
NOT built: DefectAugment's deformation and artifacts (0 / absent in the reference's call), ClaheAugment, 3-D rotations.
The 2-D setups have their own chains, batched over the ten draws of a step (augment2d.py, the key `augment2d` and `intensity`
inside it).  The synthetic labels of the second-stage setups (train.SyntheticSource) run through the same map and the same
two launches, with labels 0 outside the block (augment_labels.py, the key `label_augment`).
"""
import ctypes as C
import dataclasses
import math

import numpy as np

# what the trainer's log line names as missing: without `intensity`, and with it
NOT_BUILT = "NoiseAugment, IntensityAugment, GammaAugment, ImpulseNoiseAugment, SmoothAugment and DefectAugment of raw"
NOT_BUILT_WITH_INTENSITY = ("DefectAugment's deformation and artifacts (the 2-D setups have their own key, `augment2d`, the synthetic labels "
                            "of the second-stage setups `label_augment`)")
MAX_LATTICE_NODES = 4096   # csrc/augment.hip: 48 KiB of offsets in LDS
MAX_RADIUS = 6             # csrc/augment_intensity.hip: taps of the smoothing kernel, int(4 sigma + 0.5)
STAT_PARTS = 16            # include/bsmi.h: BSMI_AUG_STAT_PARTS


@dataclasses.dataclass(frozen=True)
class IntensityParams:
    """The arguments of the six intensity nodes; the defaults are the reference's call site (models/3d_mtlsd/train.py:117-132).
    impulse_pixel_p: the share of voxels an applied ImpulseNoiseAugment replaces.  None (the default) is what the reference
    EXECUTES, impulse_p: its node draws the locations with p, not with the pixel_p = 0.05 its call site passes.  Set the
    key to get the documented 0.05."""
    noise_p: float = 0.5
    noise_var: float = 0.01
    intensity_p: float = 0.5
    scale: tuple = (0.9, 1.1)
    shift: tuple = (-0.1, 0.1)
    gamma_p: float = 0.5
    gamma: tuple = (0.8, 1.2)
    impulse_p: float = 0.5
    impulse_pixel_p: float = None
    smooth_p: float = 0.5
    blur: tuple = (0.5, 1.5)
    prob_missing: float = 0.1
    prob_low_contrast: float = 0.1
    contrast_scale: float = 0.1

    @classmethod
    def from_config(cls, value, key="augment.intensity"):
        """The key `intensity` of the `[augment]` table: absent / false -> None, true -> the defaults, a table -> overrides.
        key: how the errors name it (the 2-D setups parse the same table as `augment2d.intensity`)."""
        if value is None or value is False:
            return None
        if value is True:
            return cls()
        if not isinstance(value, dict):
            raise ValueError(f"{key} must be true, false or a table, not {value!r}")
        names = [f.name for f in dataclasses.fields(cls)]
        unknown = sorted(set(value) - set(names))
        if unknown:
            raise ValueError(f"unknown {key} key(s) {', '.join(unknown)}; known: {', '.join(names)}")
        kw = {}
        for k, v in value.items():
            if k in ("scale", "shift", "gamma", "blur"):
                kw[k] = tuple(float(x) for x in v)
                if len(kw[k]) != 2 or not kw[k][0] <= kw[k][1] or (k != "shift" and kw[k][0] <= 0):
                    raise ValueError(f"{key}.{k} {v!r}: two numbers, low <= high" + ("" if k == "shift" else ", positive"))
                if k == "blur" and int(4.0 * kw[k][1] + 0.5) > MAX_RADIUS:
                    raise ValueError(f"{key}.blur {v!r}: sigma below {(MAX_RADIUS + 0.5) / 4} (a radius int(4 sigma + 0.5) of at most {MAX_RADIUS})")
            else:
                kw[k] = float(v)
                if k in ("noise_var", "contrast_scale"):
                    if kw[k] < 0:
                        raise ValueError(f"{key}.{k} {v!r}: not negative")
                elif kw[k] < 0 or kw[k] > 1:
                    raise ValueError(f"{key}.{k} {v!r}: a probability")
        p = cls(**kw)
        if p.prob_missing + p.prob_low_contrast > 1:
            raise ValueError(f"{key}: prob_missing + prob_low_contrast exceeds 1")
        return p


@dataclasses.dataclass(frozen=True)
class AugParams:
    """The arguments of the three nodes; the defaults are the reference's (models/3d_affs/train.py:95-104).
    control_point_spacing / jitter_sigma: world units per axis, None = the reference's voxel_size * (vs[2], vs[0], vs[0])
    and voxel_size * 2.  intensity: an IntensityParams turns on the intensity chain of raw; None (the default, also of
    `augment = true`): the geometric chain alone."""
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
    intensity: IntensityParams = None

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
            if k == "intensity":
                kw[k] = IntensityParams.from_config(v)
            elif k in ("simple", "rotate"):
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


def check_square(inp, out, key="augment"):
    """key: the train config table whose `simple` the error names (`label_augment` for the synthetic labels)"""
    if inp[1] != inp[2] or out[1] != out[2]:
        raise ValueError(f"the y/x swap of SimpleAugment (transpose_only=[1, 2]) needs square blocks, not input {list(inp)} / output {list(out)}; "
                         f"set {key}.simple = false")


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


@dataclasses.dataclass
class IntensityPlan:
    """One sample's intensity draws, in the number formats the kernels read.  A node that is not applied holds None.
    noise_sigma: float32 sqrt(noise_var).  scale, shift, gamma: float32 [D], per section (gamma already mapped to the
    exponent).  impulse_threshold: floor(q * 2^32), an int in [0, 2^32].  blur: the sigma drawn; weights: float32
    [2 radius + 1], the normalised taps.  defect: int32 [D] of 0 (unchanged), 1 / 2 (missing: the section becomes 0 / 1),
    3 (low contrast), or None where no section has a defect.  seed: the 64-bit Philox key of noise and impulse."""
    shape: tuple
    noise_sigma: float = None
    scale: np.ndarray = None
    shift: np.ndarray = None
    gamma: np.ndarray = None
    impulse_threshold: int = None
    blur: float = None
    weights: np.ndarray = None
    defect: np.ndarray = None
    contrast_scale: float = 0.1
    seed: int = 0

    @property
    def applied(self):
        """whether any node changes raw; if none does, the source takes today's sample_raw path"""
        return any(v is not None for v in (self.noise_sigma, self.scale, self.gamma, self.impulse_threshold, self.weights, self.defect))


def gamma_interval(gamma):
    """GammaAugment's draw interval: (lo', hi') with v' = (max(v, 1 / v) - 1) * (-1 if v < 1 else 1)"""
    return tuple((max(v, 1.0 / v) - 1.0) * (-1.0 if v < 1 else 1.0) for v in gamma)


def gamma_exponent(g):
    """a draw of gamma_interval -> the exponent: 1 / (1 - g) below 0, else g + 1"""
    g = np.asarray(g, dtype=np.float64)
    return np.where(g < 0, 1.0 / (1.0 - np.minimum(g, 0.0)), g + 1.0)


def gaussian_weights(sigma):
    """scipy.ndimage's taps for truncate = 4: radius int(4 sigma + 0.5), exp(-x^2 / (2 sigma^2)) normalised in float64, as float32"""
    radius = int(4.0 * float(sigma) + 0.5)
    if radius > MAX_RADIUS:
        raise ValueError(f"smoothing sigma {sigma}: a radius of {radius}, at most {MAX_RADIUS}")
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * x * x)
    return (w / w.sum()).astype(np.float32)


def draw_intensity_plan(rng, params, shape):
    """One intensity plan for a block of `shape` (D sections), every draw taken from `rng` in this order; a node whose
    probability is 0 takes no draw at all.
      1. noise:     rng.random() < noise_p
      2. intensity: rng.random() < intensity_p; if applied: rng.uniform(*scale, D), then rng.uniform(*shift, D)
      3. gamma:     rng.random() < gamma_p; if applied: rng.uniform(*gamma_interval(gamma), D), mapped by gamma_exponent
      4. impulse:   rng.random() < impulse_p
      5. smooth:    rng.random() < smooth_p; if applied: sigma = rng.uniform(*blur)
      6. defect:    if prob_missing + prob_low_contrast > 0: r = rng.random(D), then rng.random(D) < 0.5 -- the value, 0 or
                    1, a section takes if it is missing; both always, so that the stream does not depend on the outcome
      7. seed:      if noise or impulse is applied: rng.integers(0, 2^64, dtype=uint64), the Philox key of both
    """
    shape = tuple(int(v) for v in shape)
    d = shape[0]
    plan = IntensityPlan(shape, contrast_scale=float(params.contrast_scale))
    if params.noise_p > 0 and rng.random() < params.noise_p:
        plan.noise_sigma = float(np.float32(math.sqrt(params.noise_var)))
    if params.intensity_p > 0 and rng.random() < params.intensity_p:
        plan.scale = rng.uniform(*params.scale, d).astype(np.float32)
        plan.shift = rng.uniform(*params.shift, d).astype(np.float32)
    if params.gamma_p > 0 and rng.random() < params.gamma_p:
        plan.gamma = gamma_exponent(rng.uniform(*gamma_interval(params.gamma), d)).astype(np.float32)
    if params.impulse_p > 0 and rng.random() < params.impulse_p:
        q = params.impulse_p if params.impulse_pixel_p is None else params.impulse_pixel_p
        plan.impulse_threshold = int(math.floor(q * 2.0 ** 32))
    if params.smooth_p > 0 and rng.random() < params.smooth_p:
        plan.blur = float(rng.uniform(*params.blur))
        plan.weights = gaussian_weights(plan.blur)
    if params.prob_missing + params.prob_low_contrast > 0:
        r = rng.random(d)
        missing = r < params.prob_missing
        low = ~missing & (r < params.prob_missing + params.prob_low_contrast)
        mode = np.where(low, 3, 0).astype(np.int32)
        mode[missing] = np.where(rng.random(d) < 0.5, 1, 2)[missing]
        if mode.any():
            plan.defect = mode
    if plan.noise_sigma is not None or plan.impulse_threshold is not None:
        plan.seed = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
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


def sample_unit(coords_dev, crop, region=None):
    """uint8 crop -> float32 region in [0, 1]: trilinear, v / 255 -- what the intensity chain starts from"""
    import torch
    return _sample("bsmi_aug_sample_unit_f32_u8", coords_dev, crop, region, torch.uint8, torch.float32)


# ---- the intensity nodes: each changes a contiguous float32 CUDA block (D, H, W) in [0, 1] in place ----

def _block(x):
    import torch
    from . import _lib
    if x.dtype != torch.float32 or x.dim() != 3 or not x.is_cuda or not x.is_contiguous():
        raise ValueError("the block must be a contiguous float32 CUDA tensor (D, H, W)")
    return x.device.index, _lib.i64x3(x.shape), C.c_void_p(x.data_ptr()), C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)


def _per_section(x, values, dtype, what):
    """`values` (numpy or tensor, one per section) as a tensor of `dtype` on x's device"""
    import torch
    t = values if isinstance(values, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(values)).to(x.device)
    if t.dtype != dtype or tuple(t.shape) != (x.shape[0],) or t.device != x.device or not t.is_contiguous():
        raise ValueError(f"{what}: one {dtype} value per section ({x.shape[0]}) on the block's device")
    t.record_stream(torch.cuda.current_stream(x.device))
    return t


def noise(x, seed, sigma):
    """x = clip(x + sigma n), n from words 0 and 1 of Philox4x32-10(counter = voxel index, key = seed)"""
    from . import _lib
    dev, shape, ptr, stream = _block(x)
    _lib.check(_lib.lib.bsmi_aug_noise_f32(dev, shape, ptr, C.c_uint64(int(seed)), C.c_float(float(sigma)), stream))
    return x


def impulse(x, seed, threshold):
    """a voxel whose Philox word 2 < threshold (an int in [0, 2^32]) becomes (word 3 >> 8) * 2^-24"""
    from . import _lib
    dev, shape, ptr, stream = _block(x)
    _lib.check(_lib.lib.bsmi_aug_impulse_f32(dev, shape, ptr, C.c_uint64(int(seed)), C.c_uint64(int(threshold)), stream))
    return x


def section_stats(x):
    """float32 CUDA (D, 3): mean, min and max of every section, reduced in a fixed order (one block, one result)"""
    import torch
    from . import _lib
    dev, shape, ptr, stream = _block(x)
    partials = torch.empty((x.shape[0], STAT_PARTS, 3), dtype=torch.float32, device=x.device)
    stats = torch.empty((x.shape[0], 3), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib.bsmi_aug_section_stats_f32(dev, shape, ptr, C.c_void_p(partials.data_ptr()), C.c_void_p(stats.data_ptr()), stream))
    return stats


def _stats(x, stats):
    import torch
    if stats.dtype != torch.float32 or tuple(stats.shape) != (x.shape[0], 3) or stats.device != x.device or not stats.is_contiguous():
        raise ValueError("stats must be section_stats of the block: float32 (D, 3) on its device")
    return C.c_void_p(stats.data_ptr())


def intensity(x, stats, scale, shift):
    """x = clip(m_z + (x - m_z) scale_z + shift_z) with m_z = stats[z, 0]"""
    import torch
    from . import _lib
    dev, shape, ptr, stream = _block(x)
    sc, sh = _per_section(x, scale, torch.float32, "scale"), _per_section(x, shift, torch.float32, "shift")
    _lib.check(_lib.lib.bsmi_aug_intensity_f32(dev, shape, ptr, _stats(x, stats), C.c_void_p(sc.data_ptr()), C.c_void_p(sh.data_ptr()), stream))
    return x


def gamma(x, stats, exponent):
    """x = ((x - a) / (b - a))^g_z (b - a) + a with (a, b) = stats[z, 1:], where b - a > 1e-3"""
    import torch
    from . import _lib
    dev, shape, ptr, stream = _block(x)
    g = _per_section(x, exponent, torch.float32, "gamma")
    _lib.check(_lib.lib.bsmi_aug_gamma_f32(dev, shape, ptr, _stats(x, stats), C.c_void_p(g.data_ptr()), stream))
    return x


def smooth(x, weights):
    """the separable Gaussian of `weights` (float32, 2 radius + 1 normalised taps: gaussian_weights) along z, y, x, border reflect"""
    import torch
    from . import _lib
    dev, shape, ptr, stream = _block(x)
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.ndim != 1 or w.size % 2 != 1:
        raise ValueError("weights: 2 radius + 1 taps")
    tmp = torch.empty_like(x)
    _lib.check(_lib.lib.bsmi_aug_smooth_f32(dev, shape, ptr, C.c_void_p(tmp.data_ptr()), _f32(w), w.size // 2, stream))
    return x


def defect(x, stats, mode, contrast_scale, final_map=False):
    """per section mode 0: unchanged, 1 / 2: all 0 / all 1, 3: x = m_z + (x - m_z) contrast_scale; mode None: no section;
    final_map: then x = 2 x - 1"""
    import torch
    from . import _lib
    dev, shape, ptr, stream = _block(x)
    m = _per_section(x, mode, torch.int32, "defect mode") if mode is not None else None
    _lib.check(_lib.lib.bsmi_aug_defect_f32(dev, shape, ptr, _stats(x, stats) if m is not None else None,
                                            C.c_void_p(m.data_ptr()) if m is not None else None, C.c_float(float(contrast_scale)), 1 if final_map else 0, stream))
    return x


def apply_intensity(x, plan, final_map=True):
    """The chain of `plan` (an IntensityPlan) on x in [0, 1], in place, a launch per applied node and the section statistics
    its successor needs; then 2 x - 1.  A node the plan skips is not launched, so it leaves the values bit-equal."""
    if tuple(x.shape) != tuple(plan.shape):
        raise ValueError(f"block of shape {tuple(x.shape)} for a plan of {plan.shape}")
    if plan.noise_sigma is not None:
        noise(x, plan.seed, plan.noise_sigma)
    if plan.scale is not None:
        intensity(x, section_stats(x), plan.scale, plan.shift)
    if plan.gamma is not None:
        gamma(x, section_stats(x), plan.gamma)
    if plan.impulse_threshold is not None:
        impulse(x, plan.seed, plan.impulse_threshold)
    if plan.weights is not None:
        smooth(x, plan.weights)
    low = plan.defect is not None and bool((plan.defect == 3).any())
    return defect(x, section_stats(x) if low else _no_stats(x), plan.defect, plan.contrast_scale, final_map)


def _no_stats(x):
    """stats no section reads (no low-contrast section in the plan): allocated, never reduced"""
    import torch
    return torch.empty((x.shape[0], 3), dtype=torch.float32, device=x.device)


def sample_raw_intensity(coords_dev, crop, plan):
    """uint8 crop -> float32 block in [-1, 1] through the intensity chain; a plan that applies no node: sample_raw, bit for bit"""
    if plan is None or not plan.applied:
        return sample_raw(coords_dev, crop)
    return apply_intensity(sample_unit(coords_dev, crop), plan)
