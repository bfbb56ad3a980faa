"""Input augmentation of the second-stage setups on the device: what models/3d_affs_from_2d_mtlsd/train.py:110-126 and its
three siblings lay over every input array made from the obfuscated synthetic labels ("simulate noisy defected predictions"),
applied by csrc/augment_inputs.hip to one float32 array (C, D, H, W) in [0, 1] at a time, in place:

    NoiseAugment(mode="gaussian", p=0.1)
    IntensityAugment(0.9, 1.1, -0.1, 0.1, slab=(1, -1, -1, -1), p=0.5)      one scale / shift per channel
    IntensityAugment(0.9, 1.1, -0.1, 0.1, slab=(-1, 1, -1, -1), p=0.5)      one scale / shift per section
    SmoothAugment(slab=(-1, 1, -1, -1), blur_min=0.1, blur_max=1.5, p=0.5)  one sigma per section
    DefectAugment(prob_low_contrast=0.1, prob_missing=0.0, prob_deform=0.0, axis=1)

These are specified rules (restated in float64 by tests/augin_ref.py), not a transcription of gunpowder,
which is not installed where this was written: parity with the reference is in distribution, not draw by draw.

    noise      x = clip(x + sqrt(noise_var) n), n a standard normal per voxel: Philox4x32-10 on the linear index within the
               array, so every channel has its own noise (augment.noise on the array viewed as (C D, H, W))
    channel    x = clip(m_c + (x - m_c) scale_c + shift_c), m_c the channel's mean over (D, H, W)
    section    x = clip(m_z + (x - m_z) scale_z + shift_z), m_z the section's mean over (C, H, W) after `channel`
    smooth     per section, sigma_z: scipy.ndimage.gaussian_filter(x[:, z:z+1], sigma_z) -- along c, y and x (the z axis of the
               slab has length 1); taps augment.gaussian_weights(sigma_z), radius int(4 sigma + 0.5), border reflect; a section
               of radius 0 (sigma < 0.125) stays as it is, bit for bit; the result is held to [0, 1], which the exact sums never
               leave (float32 taps can add up to 1 and a few ulp)
    contrast   per section with r_z < prob_low_contrast: x = m_z + (x - m_z) contrast_scale, m_z over (C, H, W)

Declared quirks of the reference, both kept or named:
  * SmoothAugment blurs ACROSS CHANNELS: gp/smooth_augment.py:94-101 hands the 4-D slab (C, 1, H, W) to gaussian_filter with a
    scalar sigma.  `smooth_channels` (default true: what the reference executes) = false drops the c pass.
  * DefectAugment's axis=1 counts one axis and cuts another: gp/defect_augment.py:142 draws one r per index of the SPATIAL
    ROI's axis 1, which is H, and :199-202 applies index i to the 4-D data's axis 1, which is z; indices >= D select nothing.
    Here D values are drawn, one per section; the reference's surplus H - D draws act on nothing.
NOT built: DefectAugment's missing, deformed and artifact sections (0 / absent in the reference's call).  SimpleAugment,
DeformAugment and ShiftAugment of the synthetic labels have a key of their own, `label_augment` (augment_labels.py, section 7o).
"""
import ctypes as C
import dataclasses
import math

import numpy as np

from .augment import MAX_RADIUS, STAT_PARTS, gaussian_weights

MAX_CHANNELS = 16            # include/bsmi.h: BSMI_AUGIN_MAX_CHANNELS, of the smoothing pass along c
TAP_ROW = 2 * MAX_RADIUS + 1   # floats per section in the table of taps
NODES = "NoiseAugment, IntensityAugment per channel and per section, SmoothAugment per section and DefectAugment's low contrast of the inputs"


@dataclasses.dataclass(frozen=True)
class InputAugParams:
    """The arguments of the five nodes; the defaults are the reference's call site (models/3d_affs_from_2d_mtlsd/train.py:110-126).
    smooth_channels: true is what the reference EXECUTES, a blur along c as well as y and x; false blurs in the plane only."""
    noise_p: float = 0.1
    noise_var: float = 0.01
    channel_intensity_p: float = 0.5
    section_intensity_p: float = 0.5
    scale: tuple = (0.9, 1.1)
    shift: tuple = (-0.1, 0.1)
    smooth_p: float = 0.5
    blur: tuple = (0.1, 1.5)
    smooth_channels: bool = True
    prob_low_contrast: float = 0.1
    contrast_scale: float = 0.1

    @classmethod
    def from_config(cls, value, key="input_augment"):
        """The train TOML key `input_augment`: absent / false -> None (today's path), true -> the defaults, a table -> overrides."""
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
            if k in ("scale", "shift", "blur"):
                kw[k] = tuple(float(x) for x in v)
                if len(kw[k]) != 2 or not kw[k][0] <= kw[k][1] or (k != "shift" and kw[k][0] <= 0):
                    raise ValueError(f"{key}.{k} {v!r}: two numbers, low <= high" + ("" if k == "shift" else ", positive"))
                if k == "blur" and int(4.0 * kw[k][1] + 0.5) > MAX_RADIUS:
                    raise ValueError(f"{key}.blur {v!r}: sigma below {(MAX_RADIUS + 0.5) / 4} (a radius int(4 sigma + 0.5) of at most {MAX_RADIUS})")
            elif k == "smooth_channels":
                if not isinstance(v, bool):
                    raise ValueError(f"{key}.{k} {v!r}: true or false")
                kw[k] = v
            else:
                kw[k] = float(v)
                if k in ("noise_var", "contrast_scale"):
                    if kw[k] < 0:
                        raise ValueError(f"{key}.{k} {v!r}: not negative")
                elif kw[k] < 0 or kw[k] > 1:
                    raise ValueError(f"{key}.{k} {v!r}: a probability")
        return cls(**kw)


@dataclasses.dataclass
class InputPlan:
    """One array's draws, in the number formats the kernels read.  A node that is not applied holds None.
    noise_sigma: float32 sqrt(noise_var).  channel_scale / channel_shift: float32 [C]; section_scale / section_shift: float32 [D].
    sigma: the D sigmas drawn (float64); weights: float32 [D][13], row z the 2 radius[z] + 1 normalised taps of sigma[z], zeros
    after them; radius: int32 [D].  low_contrast: int32 [D] of 0 (unchanged) and 3 (low contrast: the mode number of the
    intensity chain of raw), or None where no section is drawn.  seed: the 64-bit Philox key of noise."""
    shape: tuple
    noise_sigma: float = None
    channel_scale: np.ndarray = None
    channel_shift: np.ndarray = None
    section_scale: np.ndarray = None
    section_shift: np.ndarray = None
    sigma: np.ndarray = None
    weights: np.ndarray = None
    radius: np.ndarray = None
    smooth_channels: bool = True
    low_contrast: np.ndarray = None
    contrast_scale: float = 0.1
    seed: int = 0

    @property
    def applied(self):
        """whether any node changes the array"""
        smooths = self.radius is not None and bool(self.radius.any())
        return smooths or any(v is not None for v in (self.noise_sigma, self.channel_scale, self.section_scale, self.low_contrast))


def section_taps(sigma):
    """(weights float32 [D][13], radius int32 [D]) of the D sigmas: row z holds augment.gaussian_weights(sigma[z]), zeros after them"""
    sigma = np.asarray(sigma, dtype=np.float64).ravel()
    weights, radius = np.zeros((sigma.size, TAP_ROW), dtype=np.float32), np.zeros(sigma.size, dtype=np.int32)
    for z, s in enumerate(sigma):
        w = gaussian_weights(s)
        weights[z, :w.size], radius[z] = w, w.size // 2
    return weights, radius


def draw_input_plan(rng, params, shape4):
    """One plan for an array of `shape4` = (C, D, H, W), every draw taken from `rng` (a numpy Generator) in this order; a node
    whose probability is 0 takes no draw at all.
      1. noise:    rng.random() < noise_p
      2. channel:  rng.random() < channel_intensity_p; if applied: rng.uniform(*scale, C), then rng.uniform(*shift, C)
      3. section:  rng.random() < section_intensity_p; if applied: rng.uniform(*scale, D), then rng.uniform(*shift, D)
      4. smooth:   rng.random() < smooth_p; if applied: rng.uniform(*blur, D), one sigma per section
      5. contrast: if prob_low_contrast > 0: r = rng.random(D); section z is low in contrast iff r_z < prob_low_contrast
      6. seed:     if noise is applied: rng.integers(0, 2^64, dtype=uint64), the Philox key
    """
    shape4 = tuple(int(v) for v in shape4)
    if len(shape4) != 4:
        raise ValueError(f"an input array is (C, D, H, W), not {shape4}")
    c, d = shape4[:2]
    plan = InputPlan(shape4, smooth_channels=bool(params.smooth_channels), contrast_scale=float(params.contrast_scale))
    if params.noise_p > 0 and rng.random() < params.noise_p:
        plan.noise_sigma = float(np.float32(math.sqrt(params.noise_var)))
    if params.channel_intensity_p > 0 and rng.random() < params.channel_intensity_p:
        plan.channel_scale = rng.uniform(*params.scale, c).astype(np.float32)
        plan.channel_shift = rng.uniform(*params.shift, c).astype(np.float32)
    if params.section_intensity_p > 0 and rng.random() < params.section_intensity_p:
        plan.section_scale = rng.uniform(*params.scale, d).astype(np.float32)
        plan.section_shift = rng.uniform(*params.shift, d).astype(np.float32)
    if params.smooth_p > 0 and rng.random() < params.smooth_p:
        plan.sigma = rng.uniform(*params.blur, d)
        plan.weights, plan.radius = section_taps(plan.sigma)
    if params.prob_low_contrast > 0:
        low = rng.random(d) < params.prob_low_contrast
        if low.any():
            plan.low_contrast = np.where(low, 3, 0).astype(np.int32)
    if plan.noise_sigma is not None:
        plan.seed = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
    return plan


# ---- the nodes: each changes a contiguous float32 CUDA array (C, D, H, W) in [0, 1] in place ----

def _array(x):
    import torch
    from . import _lib
    if x.dtype != torch.float32 or x.dim() != 4 or not x.is_cuda or not x.is_contiguous():
        raise ValueError("the array must be a contiguous float32 CUDA tensor (C, D, H, W)")
    return x.device.index, _lib.i64x4(x.shape), C.c_void_p(x.data_ptr()), C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)


def _table(x, values, dtype, shape, what):
    """`values` (numpy or tensor) as a contiguous tensor of `dtype` and `shape` on x's device; the caller holds it until its launch
    is queued (a block freed earlier goes back to the allocator and into the next table)"""
    import torch
    t = values if isinstance(values, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(values)).to(x.device)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != x.device or not t.is_contiguous():
        raise ValueError(f"{what}: {dtype} of shape {tuple(shape)} on the array's device")
    t.record_stream(torch.cuda.current_stream(x.device))
    return t


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _groups(x, axis):
    if axis not in (0, 1):
        raise ValueError(f"axis {axis!r}: 0 (per channel) or 1 (per section)")
    return x.shape[axis]


def noise(x, seed, sigma):
    """x = clip(x + sigma n); the Philox counter is the linear index within the array: augment.noise on the view (C D, H, W)"""
    from . import augment
    _array(x)
    augment.noise(x.view(x.shape[0] * x.shape[1], x.shape[2], x.shape[3]), seed, sigma)
    return x


def group_mean(x, axis):
    """float32 CUDA (C,) for axis 0 -- the mean of every channel over (D, H, W) -- or (D,) for axis 1 -- of every section over
    (C, H, W): plane sums in a fixed order, the planes of a group added in index order (one array, one result)"""
    import torch
    from . import _lib
    dev, shape, ptr, stream = _array(x)
    work = torch.empty(x.shape[0] * x.shape[1] * (STAT_PARTS * 3 + 3), dtype=torch.float32, device=x.device)
    mean = torch.empty(_groups(x, axis), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib.bsmi_augin_group_mean_f32(dev, shape, ptr, C.c_void_p(work.data_ptr()), int(axis), C.c_void_p(mean.data_ptr()), stream))
    return mean


def intensity(x, mean, scale, shift, axis):
    """x = clip(m_g + (x - m_g) scale_g + shift_g), g the channel (axis 0) or the section (axis 1)"""
    import torch
    from . import _lib
    dev, shape, ptr, stream = _array(x)
    n = (_groups(x, axis),)
    m, sc, sh = _table(x, mean, torch.float32, n, "mean"), _table(x, scale, torch.float32, n, "scale"), _table(x, shift, torch.float32, n, "shift")
    _lib.check(_lib.lib.bsmi_augin_intensity_f32(dev, shape, ptr, _ptr(m), _ptr(sc), _ptr(sh), int(axis), stream))
    return x


def smooth(x, weights, radius, channels=True):
    """per section z the separable Gaussian of weights[z] (float32 (D, 13), the first 2 radius[z] + 1 normalised taps: section_taps)
    along c -- unless channels is false --, y and x, border reflect; a section of radius 0 is not touched"""
    import torch
    from . import _lib
    dev, shape, ptr, stream = _array(x)
    d = x.shape[1]
    if not isinstance(radius, torch.Tensor):
        r = np.asarray(radius)
        if r.shape != (d,) or r.min() < 0 or r.max() > MAX_RADIUS:
            raise ValueError(f"radius: one per section ({d}), 0 .. {MAX_RADIUS}")
    if channels and x.shape[0] > MAX_CHANNELS:
        raise ValueError(f"smoothing along c holds a column of at most {MAX_CHANNELS} channels, not {x.shape[0]}")
    tmp, w, r = torch.empty_like(x), _table(x, weights, torch.float32, (d, TAP_ROW), "weights"), _table(x, radius, torch.int32, (d,), "radius")
    _lib.check(_lib.lib.bsmi_augin_smooth_f32(dev, shape, ptr, _ptr(tmp), _ptr(w), _ptr(r), 1 if channels else 0, stream))
    return x


def contrast(x, mean, mode, contrast_scale):
    """a section of mode 3 becomes x = m_z + (x - m_z) contrast_scale with m_z = mean[z] (group_mean, axis 1); mode 0: not touched"""
    import torch
    from . import _lib
    dev, shape, ptr, stream = _array(x)
    d = (x.shape[1],)
    m, md = _table(x, mean, torch.float32, d, "mean"), _table(x, mode, torch.int32, d, "mode")
    _lib.check(_lib.lib.bsmi_augin_contrast_f32(dev, shape, ptr, _ptr(m), _ptr(md), C.c_float(float(contrast_scale)), stream))
    return x


def _pack(x, plan):
    """every table of `plan` in ONE transfer: {name: tensor on x's device}, int32 tables riding as their bits"""
    import torch
    parts = [(k, getattr(plan, k)) for k in ("channel_scale", "channel_shift", "section_scale", "section_shift", "weights", "radius", "low_contrast")]
    parts = [(k, np.ascontiguousarray(v)) for k, v in parts if v is not None]
    if not parts:
        return {}
    flat = torch.from_numpy(np.concatenate([v.view(np.float32).ravel() for _, v in parts])).to(x.device)
    flat.record_stream(torch.cuda.current_stream(x.device))
    out, at = {}, 0
    for k, v in parts:
        t = flat[at:at + v.size].view(v.shape)
        out[k] = t.view(torch.int32) if v.dtype == np.int32 else t
        at += v.size
    return out


def apply_inputs(x, plan):
    """The chain of `plan` (an InputPlan) on x, in place: a launch per applied node and the group means it reads, taken of the
    array as it is at that point.  A node the plan skips is not launched, so it leaves the values bit-equal."""
    if tuple(x.shape) != tuple(plan.shape):
        raise ValueError(f"array of shape {tuple(x.shape)} for a plan of {plan.shape}")
    t = _pack(x, plan)
    if plan.noise_sigma is not None:
        noise(x, plan.seed, plan.noise_sigma)
    if plan.channel_scale is not None:
        intensity(x, group_mean(x, 0), t["channel_scale"], t["channel_shift"], 0)
    if plan.section_scale is not None:
        intensity(x, group_mean(x, 1), t["section_scale"], t["section_shift"], 1)
    if plan.radius is not None and plan.radius.any():
        smooth(x, t["weights"], t["radius"], plan.smooth_channels)
    if plan.low_contrast is not None:
        contrast(x, group_mean(x, 1), t["low_contrast"], plan.contrast_scale)
    return x
