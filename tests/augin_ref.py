"""numpy / scipy restatement in float64 of the input augmentation of the second-stage setups (bootstrapper_amd/augment_inputs.py,
csrc/augment_inputs.hip), the gates of the comparisons, the comparisons themselves -- shared by the GPU
tests and the CPU tests, which run them on a float32 emulation with injected faults -- and the test cases.

An array is (C, D, H, W) float32 in [0, 1]: channels on axis 0, sections on axis 1.  Every launch is judged on ITS OWN input:
the array before the launch and, where the node reads them, the group means, both as the device left them, go through the
float64 rule, and the array after the launch is compared with that.

The gates.  The per-voxel device code is that of the intensity chain of raw (csrc/augment_intensity.h), so the gates of
tests/intensity_ref.py hold as derived there and are imported: NOISE_GATE (noise), intensity_gate (the two intensity nodes),
contrast_gate (low contrast) and SMOOTH_GATE (three passes -- here c, y, x -- of at most 13 taps of non-negative terms each:
the same derivation).  eps = 2^-24, bounds first order in eps times (1 + 2^-10).

  group mean   A plane's mean is taken exactly as the section statistics of the intensity chain take it, so it is within
               mean_gate of the exact one: (k + 24) eps relative, k = ceil(ceil(H W / 16) / 256).  A group adds the means of its
               P planes (P = D for a channel, C for a section), all non-negative, in index order: P - 1 additions, each one
               rounding of a partial sum that is at most the total, then one division by P: P eps more, relative to the group's
               mean.  |mean - exact| <= (k + 24 + P) eps mean.                                 group_mean_gate(shape, axis, mean)
  radius-0 sections of the smoothing, sections that are not low in contrast, skipped nodes, two runs of one plan: bit for bit.
"""
import numpy as np
import scipy.ndimage

import intensity_ref as R3
from intensity_ref import EPS, SLACK, NOISE_GATE, SMOOTH_GATE, contrast_gate, intensity_gate, mean_gate, worst  # noqa: F401

f32 = np.float32


def group_mean_gate(shape, axis, mean):
    planes = shape[1] if axis == 0 else shape[0]
    return mean_gate(shape[1:], mean) + planes * EPS * np.abs(mean) * SLACK


# ---- the rules, float64, each on the float32 array (and means) it is given ----

def _grp(v, axis):
    v = np.asarray(v, dtype=np.float64)
    return v[:, None, None, None] if axis == 0 else v[None, :, None, None]


def group_mean(x, axis):
    return np.asarray(x, dtype=np.float64).mean(axis=(1, 2, 3) if axis == 0 else (0, 2, 3))


def noise(x, seed, sigma):
    """the counter is the linear index within the array: every channel has its own noise"""
    return R3.noise(x, seed, sigma)


def intensity(x, mean, scale, shift, axis):
    m = _grp(mean, axis)
    return np.clip(m + (x.astype(np.float64) - m) * _grp(scale, axis) + _grp(shift, axis), 0.0, 1.0)


def smooth(x, sigma, channels=True):
    """literally the reference's call per section: gaussian_filter on the 4-D slab (C, 1, H, W) with a scalar sigma, which filters
    along c as well; smooth_channels = false: sigma (0, 0, s, s)"""
    y = np.empty(x.shape, dtype=np.float64)
    for z, s in enumerate(np.asarray(sigma, dtype=np.float64)):
        y[:, z:z + 1] = scipy.ndimage.gaussian_filter(x[:, z:z + 1].astype(np.float64), float(s) if channels else (0.0, 0.0, float(s), float(s)),
                                                      mode="reflect")
    return y


def contrast(x, mean, mode, contrast_scale):
    x = x.astype(np.float64)
    m = _grp(mean, 1)
    return np.where(np.asarray(mode)[None, :, None, None] == 3, m + (x - m) * float(contrast_scale), x)


# ---- the chain, stage by stage, through a backend ----
# A backend `ops` has noise / group_mean / intensity / smooth / contrast, each from numpy float32 arrays to a new numpy float32
# array, and chain(x, plan): the fused path, all of it at once.

def smooths(plan):
    return plan.radius is not None and bool(plan.radius.any())


def staged(ops, x0, plan):
    """the chain of `plan` in the specified order, one call per node: [(node, array before, array or means after, the means the
    node read or None)]"""
    rec, x = [], np.array(x0, dtype=np.float32)

    def put(node, y, mean=None):
        nonlocal x
        rec.append((node, x, y, mean))
        if not node.endswith("_mean"):
            x = y

    if plan.noise_sigma is not None:
        put("noise", ops.noise(x, plan.seed, plan.noise_sigma))
    if plan.channel_scale is not None:
        m = ops.group_mean(x, 0)
        put("channel_mean", m)
        put("channel", ops.intensity(x, m, plan.channel_scale, plan.channel_shift, 0), m)
    if plan.section_scale is not None:
        m = ops.group_mean(x, 1)
        put("section_mean", m)
        put("section", ops.intensity(x, m, plan.section_scale, plan.section_shift, 1), m)
    if smooths(plan):
        put("smooth", ops.smooth(x, plan.weights, plan.radius, plan.smooth_channels))
    if plan.low_contrast is not None:
        m = ops.group_mean(x, 1)
        put("contrast_mean", m)
        put("contrast", ops.contrast(x, m, plan.low_contrast, plan.contrast_scale), m)
    return rec


def check(rec, plan, chain_out, show=print):
    """Every comparison of one staged run; raises AssertionError naming the node.  Returns {node: largest |got - float64|}."""
    shape, seen = plan.shape, {}
    for node, before, after, mean in rec:
        assert after.dtype == np.float32, f"{node}: dtype"
        if node.endswith("_mean"):
            axis = 0 if node == "channel_mean" else 1
            want = group_mean(before, axis)
            assert after.shape == want.shape, f"{node}: one mean per group"
            gate = group_mean_gate(shape, axis, want)
        elif node == "noise":
            want, gate = noise(before, plan.seed, plan.noise_sigma), NOISE_GATE
        elif node == "channel":
            want, gate = intensity(before, mean, plan.channel_scale, plan.channel_shift, 0), intensity_gate(plan.channel_scale, plan.channel_shift)
        elif node == "section":
            want, gate = intensity(before, mean, plan.section_scale, plan.section_shift, 1), intensity_gate(plan.section_scale, plan.section_shift)
        elif node == "smooth":
            want = smooth(before, plan.sigma, plan.smooth_channels)
            gate = np.where(plan.radius > 0, SMOOTH_GATE, 0.0)[None, :, None, None]        # a section of radius 0: bit for bit
        else:
            want = contrast(before, mean, plan.low_contrast, plan.contrast_scale)
            gate = np.where(plan.low_contrast == 3, contrast_gate(plan.contrast_scale), 0.0)[None, :, None, None]   # untouched sections: exact
        diff, ratio = worst(after, want, gate)
        show(f"{node} {shape}: largest |got - float64| {diff:.3e}, {ratio:.3f} of its gate")
        assert ratio <= 1.0, f"{node}: {diff:.3e} is {ratio:.3f} of its gate"
        if node in ("noise", "channel", "section", "smooth"):   # the clipped nodes, and the smoothing, which holds its sums to [0, 1]
            assert after.min() >= 0.0 and after.max() <= 1.0, f"{node}: leaves [0, 1]"
        seen[node] = max(seen.get(node, 0.0), diff)
    last = rec[-1][2] if rec else chain_out
    assert np.array_equal(chain_out, last), "chain: the fused path differs from its nodes run one by one in the specified order"
    return seen


# ---- a float32 emulation of the launches, with faults to inject (tests/test_augin_cpu.py) ----

FAULTS = ("axis_swapped",            # the channel node indexes its tables by the section
          "plane_mean",              # a group's mean is the mean of its first plane
          "no_c_pass",               # smoothing in the plane only while smooth_channels is on
          "one_sigma",               # the taps of section 0 for every section
          "mirror_c",                # border `mirror` (d c b | a b c d) along c
          "contrast_plane_mean",     # low contrast pulls every plane towards its own mean
          "noise_per_channel",       # the Philox counter restarts with every channel
          "stale_section_mean")      # the section node reads the means from before the channel node


class Emulation:
    """the launches in numpy float32, operation by operation (the math functions and the means: float64, rounded once);
    fault: one of FAULTS or None"""

    def __init__(self, fault=None):
        assert fault is None or fault in FAULTS
        self.fault = fault
        self._before_channel = None

    def noise(self, x, seed, sigma):
        counters = np.arange(x.size)
        if self.fault == "noise_per_channel":
            counters = counters % (x.size // x.shape[0])
        n = R3.normals(R3.philox(counters, seed)).reshape(x.shape).astype(f32)
        return np.clip(x + f32(sigma) * n, 0, 1).astype(f32)

    def group_mean(self, x, axis):
        if self.fault == "stale_section_mean" and axis == 1 and self._before_channel is not None:
            x, self._before_channel = self._before_channel, None
        if self.fault == "plane_mean":
            planes = x[:, 0] if axis == 0 else x[0]
            return planes.astype(np.float64).mean(axis=(1, 2)).astype(f32)
        return group_mean(x, axis).astype(f32)

    def intensity(self, x, mean, scale, shift, axis):
        if axis == 0:
            self._before_channel = x
        if self.fault == "axis_swapped" and axis == 0:
            pick = np.arange(x.shape[1]) % x.shape[0]
            mean, scale, shift, axis = mean[pick], scale[pick], shift[pick], 1
        g = (lambda v: v[:, None, None, None]) if axis == 0 else (lambda v: v[None, :, None, None])
        return np.clip(g(mean) + (x - g(mean)) * g(scale) + g(shift), 0, 1).astype(f32)

    def smooth(self, x, weights, radius, channels):
        y = x.copy()
        for z in range(x.shape[1]):
            zt = 0 if self.fault == "one_sigma" else z
            r = int(radius[zt])
            if r == 0:
                continue
            w = weights[zt, :2 * r + 1].astype(np.float64)
            sec = x[:, z]
            for axis in range(3):
                if axis == 0 and (not channels or self.fault == "no_c_pass"):
                    continue
                sec = scipy.ndimage.correlate1d(sec, w, axis=axis, output=f32, mode="mirror" if axis == 0 and self.fault == "mirror_c" else "reflect")
            y[:, z] = np.clip(sec, 0, 1)   # held to [0, 1], which the exact sums never leave
        return y

    def contrast(self, x, mean, mode, contrast_scale):
        m = mean[None, :, None, None]
        if self.fault == "contrast_plane_mean":
            m = x.astype(np.float64).mean(axis=(2, 3), keepdims=True).astype(f32)
        return np.where(mode[None, :, None, None] == 3, m + (x - m) * f32(contrast_scale), x).astype(f32)

    def chain(self, x, plan):
        rec = staged(self, x, plan)
        return rec[-1][2] if rec else np.array(x, dtype=np.float32)


# ---- the cases of tests/test_augin_gpu.py ----

ARRAYS = {"6x3x24x40": (6, 3, 24, 40),    # two tile rows of the y/x pass
          "2x2x17x70": (2, 2, 17, 70),    # C far below radius 6: the reflection along c is repeated; two tile columns
          "10x1x7x5": (10, 1, 7, 5),      # one section; H and W below the radius
          "3x4x20x20": (3, 4, 20, 20)}
NODES = ("noise", "channel", "section", "smooth", "contrast")
CASES = [(a, n) for a in ARRAYS for n in ("all",) + NODES + ("smooth_plane",)]   # smooth_plane: all nodes, smooth_channels = false
SIGMAS = (1.5, 0.1, 0.5)   # radius 6, 0 and 2, cycling over the sections


def build_array(shape, seed=5):
    """float32 in [0, 1]: random, every channel holding an exact 0 and an exact 1 in its last section (range 1); the plane
    (c, z) = (0, 0) constant 0.5; with more than two sections, section 1 all zero in every channel (padding beyond the volume)"""
    rng = np.random.default_rng(seed)
    x = rng.random(shape, dtype=np.float32)
    x[:, -1, 0, 0], x[:, -1, -1, -1] = 0.0, 1.0
    if shape[1] > 2:
        x[:, 1] = 0.0
    x[0, 0] = 0.5
    return x


def build_plan(shape, nodes="all", seed=7):
    """A plan that applies `nodes` ("all", one name, or "smooth_plane"), from its own seeded stream -- the launches are tested
    on their inputs, whatever drew them.  The section sigmas cycle SIGMAS; the even sections are low in contrast."""
    from bootstrapper_amd.augment_inputs import InputPlan, section_taps
    rng = np.random.default_rng(seed)
    c, d = shape[:2]
    on = (lambda n: True) if nodes in ("all", "smooth_plane") else (lambda n: n == nodes)
    plan = InputPlan(tuple(shape), contrast_scale=0.1, smooth_channels=nodes != "smooth_plane", seed=int(rng.integers(0, 2 ** 64, dtype=np.uint64)))
    cs, ch = rng.uniform(0.9, 1.1, c).astype(f32), rng.uniform(-0.1, 0.1, c).astype(f32)
    ss, sh = rng.uniform(0.9, 1.1, d).astype(f32), rng.uniform(-0.1, 0.1, d).astype(f32)
    if on("noise"):
        plan.noise_sigma = float(f32(0.1))
    if on("channel"):
        plan.channel_scale, plan.channel_shift = cs, ch
    if on("section"):
        plan.section_scale, plan.section_shift = ss, sh
    if on("smooth"):
        plan.sigma = np.array([SIGMAS[z % 3] for z in range(d)], dtype=np.float64)
        plan.weights, plan.radius = section_taps(plan.sigma)
    if on("contrast"):
        plan.low_contrast = np.array([3 if z % 2 == 0 else 0 for z in range(d)], dtype=np.int32)
    return plan
