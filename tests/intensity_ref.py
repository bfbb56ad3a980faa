"""numpy / scipy restatement in float64 of the intensity training augmentation (bootstrapper_amd/augment.py,
csrc/augment_intensity.hip), the gates of the comparisons, the comparisons themselves -- shared by the
GPU tests and the CPU tests, which run them on a float32 emulation with injected faults -- and the test cases.

Every launch is judged on ITS OWN input: the block before the launch and, where the node reads them, the section statistics,
both as the device left them, go through the float64 rule, and the block after the launch is compared with that.

The gates.  eps = 2^-24 is the unit roundoff of float32; bounds are first order in eps, times (1 + 2^-10) for the higher
orders.  Values lie in [0, 1]; a fused multiply-add rounds once where the bound counts twice, so contraction only helps.

  statistics   min and max are exact.  A section's sum has N = H W non-negative terms: a thread adds k = ceil(ceil(N / 16)
               / 256) of them one after the other, eight tree levels and sixteen partials follow, then one division:
               |mean - exact| <= (k + 24) eps mean.                                          mean_gate(shape, mean)
  intensity    m + (x - m) s + sh: the difference (<= 1 in magnitude), the product, two sums, each one rounding of a value of at
               most 1 + |s| + |sh|; the clip is 1-Lipschitz:  4 eps (1 + |s| + |sh|).        intensity_gate(scale, shift)
  low contrast m + (x - m) c: three roundings of values of at most 1 + c:  3 eps (1 + c).    contrast_gate(c)
  smooth       the taps are the float64 taps rounded to float32 (eps per tap, relative); a pass is a sum of at most 13 products
               of non-negative terms: at most (13 + 1) eps max|x| per pass, and the passes' errors go through convex
               combinations: 42 eps for the three of them.                                   SMOOTH_GATE
  noise, gamma the rules go through logf, cospif and powf, for which no accuracy statement is at hand where this was written.
               As agreed for that case, the gate is 4 x the largest |device - float64| observed over the cases of
               tests/test_intensity_gpu.py on an MI355X: noise 4.4632e-08, gamma 9.0849e-08 (both below
               two ulp of a value near 1).                                                                NOISE_GATE, GAMMA_GATE
  impulse, missing sections, the final 2 x - 1 (2 x is exact, so one rounding: numpy's float32 gives the same bits), skipped
  nodes, two runs of one plan: bit for bit.
"""
import numpy as np
import scipy.ndimage

EPS = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
SMOOTH_GATE = 42 * EPS * SLACK
OBSERVED = {"noise": 4.4632e-08, "gamma": 9.0849e-08}   # largest |device - float64| on an MI355X over CASES
NOISE_GATE = 4 * OBSERVED["noise"]
GAMMA_GATE = 4 * OBSERVED["gamma"]
M32 = np.uint64(0xFFFFFFFF)
KNOWN_ANSWER = (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)   # Random123 kat_vectors: philox4x32-10, counter 0, key 0


def mean_gate(shape, mean):
    n = shape[1] * shape[2]
    k = -(-(-(-n // 16)) // 256)
    return (k + 24) * EPS * np.abs(mean) * SLACK


def intensity_gate(scale, shift):
    return 4 * EPS * (1.0 + float(np.abs(scale).max()) + float(np.abs(shift).max())) * SLACK


def contrast_gate(c):
    return 3 * EPS * (1.0 + abs(float(c))) * SLACK


# ---- Philox4x32-10 and what is made of its words ----

def philox(counter, seed):
    """(4, N) uint32 words o0 .. o3 of Philox4x32-10 on the counters (counter, 0, 0, 0) with key (seed low, seed high), in uint64 arithmetic"""
    c = [np.asarray(counter, dtype=np.uint64).ravel().copy()] + [np.zeros(np.size(counter), dtype=np.uint64) for _ in range(3)]
    k0, k1 = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64((int(seed) >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]   # 32 x 32 bits: fits 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c).astype(np.uint32)


def normals(words):
    """n = sqrt(-2 ln u1) cos(2 pi u2) in float64, u1 = ((o0 >> 8) + 1) 2^-24, u2 = (o1 >> 8) 2^-24"""
    u1 = ((words[0] >> 8).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (words[1] >> 8).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def impulses(words, threshold, word=2):
    """(mask, values): a voxel is an impulse iff o2 < threshold (an int in [0, 2^32]); its value (o3 >> 8) 2^-24, exact in float32"""
    return words[word].astype(np.uint64) < np.uint64(threshold), ((words[3] >> 8).astype(np.float64) * 2.0 ** -24).astype(np.float32)


# ---- the rules, float64, each on the float32 block (and statistics) it is given ----

def stats(x):
    x = np.asarray(x, dtype=np.float64)
    return np.stack([x.mean(axis=(1, 2)), x.min(axis=(1, 2)), x.max(axis=(1, 2))], axis=1)


def _sec(v):
    return np.asarray(v, dtype=np.float64)[:, None, None]


def noise(x, seed, sigma):
    n = normals(philox(np.arange(x.size), seed)).reshape(x.shape)
    return np.clip(x.astype(np.float64) + float(sigma) * n, 0.0, 1.0)


def intensity(x, st, scale, shift):
    m = _sec(st[:, 0])
    return np.clip(m + (x.astype(np.float64) - m) * _sec(scale) + _sec(shift), 0.0, 1.0)


def gamma(x, st, g):
    a, b = _sec(st[:, 1]), _sec(st[:, 2])
    x = x.astype(np.float64)
    r = np.where(b - a > 1e-3, b - a, 1.0)
    y = np.clip((x - a) / r, 0.0, None) ** _sec(g) * r + a
    return np.where(b - a > 1e-3, y, x)


def impulse(x, seed, threshold):
    mask, val = impulses(philox(np.arange(x.size), seed), threshold)
    return np.where(mask.reshape(x.shape), val.reshape(x.shape), x)


def smooth(x, sigma):
    """literally the reference's call: SmoothAugment with slab = None filters all three axes at once"""
    return scipy.ndimage.gaussian_filter(x.astype(np.float64), sigma, mode="reflect")


def defect(x, st, mode, contrast_scale):
    x = x.astype(np.float64)
    if mode is None:
        return x
    md = np.asarray(mode)[:, None, None]
    m = _sec(st[:, 0]) if st is not None else 0.0
    return np.where(md == 1, 0.0, np.where(md == 2, 1.0, np.where(md == 3, m + (x - m) * float(contrast_scale), x)))


# ---- the chain, stage by stage, through a backend ----
# A backend `ops` has noise / stats / intensity / gamma / impulse / smooth / defect, each from numpy float32 blocks to a new
# numpy float32 block, and chain(x, plan): the fused path, all of it at once, before the final map.

def staged(ops, x0, plan):
    """the chain of `plan` in the specified order, one call per node: [(node, block before, block or statistics after,
    the statistics the node read or None)]"""
    rec, x = [], np.array(x0, dtype=np.float32)

    def put(node, y, st=None):
        nonlocal x
        rec.append((node, x, y, st))
        if node != "stats":
            x = y

    if plan.noise_sigma is not None:
        put("noise", ops.noise(x, plan.seed, plan.noise_sigma))
    if plan.scale is not None:
        st = ops.stats(x)
        put("stats", st)
        put("intensity", ops.intensity(x, st, plan.scale, plan.shift), st)
    if plan.gamma is not None:
        st = ops.stats(x)
        put("stats", st)
        put("gamma", ops.gamma(x, st, plan.gamma), st)
    if plan.impulse_threshold is not None:
        put("impulse", ops.impulse(x, plan.seed, plan.impulse_threshold))
    if plan.weights is not None:
        put("smooth", ops.smooth(x, plan.weights))
    st = None
    if plan.defect is not None and (plan.defect == 3).any():
        st = ops.stats(x)
        put("stats", st)
    put("defect", ops.defect(x, st, plan.defect, plan.contrast_scale), st)
    return rec


def worst(got, want, gate):
    """(largest |got - want|, largest |got - want| / gate over the entries with a positive gate); raises where a zero gate is exceeded"""
    diff = np.abs(np.asarray(got, dtype=np.float64) - want)
    gate = np.broadcast_to(np.asarray(gate, dtype=np.float64), diff.shape)
    assert (diff[gate == 0] == 0).all(), "differs where the rule is exact"
    pos = gate > 0
    return float(diff.max()), float((diff[pos] / gate[pos]).max()) if pos.any() else 0.0


def check(rec, plan, chain_out, show=print):
    """Every comparison of one staged run; raises AssertionError naming the node.  Returns {node: largest |got - float64|}."""
    shape, seen = plan.shape, {}
    for node, before, after, st in rec:
        if node == "stats":
            want = stats(before)
            assert np.array_equal(after[:, 1:], want[:, 1:].astype(np.float32)), "stats: section extrema"
            gate = np.zeros_like(want)
            gate[:, 0] = mean_gate(shape, want[:, 0])
        elif node == "noise":
            want, gate = noise(before, plan.seed, plan.noise_sigma), NOISE_GATE
        elif node == "intensity":
            want, gate = intensity(before, st, plan.scale, plan.shift), intensity_gate(plan.scale, plan.shift)
        elif node == "gamma":
            want, gate = gamma(before, st, plan.gamma), GAMMA_GATE
            flat = st[:, 2] - st[:, 1] <= 1e-3
            assert np.array_equal(after[flat], before[flat]), "gamma: a section without range must stay as it is"
        elif node == "impulse":
            want, gate = impulse(before, plan.seed, plan.impulse_threshold), 0.0
        elif node == "smooth":
            want, gate = smooth(before, plan.blur), SMOOTH_GATE
        else:
            want = defect(before, st, plan.defect, plan.contrast_scale)
            md = np.zeros(shape[0], dtype=np.int32) if plan.defect is None else plan.defect
            gate = np.where(md == 3, contrast_gate(plan.contrast_scale), 0.0)[:, None, None]   # missing and untouched sections: exact
        diff, ratio = worst(after, want, gate)
        show(f"{node} {shape}: largest |got - float64| {diff:.3e}, {ratio:.3f} of its gate")
        assert ratio <= 1.0, f"{node}: {diff:.3e} is {ratio:.3f} of its gate"
        if node != "stats":
            assert after.dtype == np.float32 and after.min() >= 0.0 and after.max() <= 1.0, f"{node}: leaves [0, 1]"
        seen[node] = max(seen.get(node, 0.0), diff)
    assert np.array_equal(chain_out, rec[-1][2]), "chain: the fused path differs from its nodes run one by one in the specified order"
    return seen


# ---- a float32 emulation of the launches, with faults to inject (tests/test_intensity_cpu.py) ----

FAULTS = ("block_mean", "gamma_unnormalised", "mirror_border", "noise_unclipped", "defect_before_smooth", "impulse_wrong_word")
f32 = np.float32


class Emulation:
    """the launches in numpy float32, operation by operation (the math functions: float64, rounded once); fault: one of FAULTS or None"""

    def __init__(self, fault=None):
        assert fault is None or fault in FAULTS
        self.fault = fault

    def noise(self, x, seed, sigma):
        n = normals(philox(np.arange(x.size), seed)).reshape(x.shape).astype(f32)
        y = x + f32(sigma) * n
        return y.astype(f32) if self.fault == "noise_unclipped" else np.clip(y, 0, 1).astype(f32)

    def stats(self, x):
        st = stats(x).astype(f32)
        if self.fault == "block_mean":
            st[:, 0] = f32(x.astype(np.float64).mean())
        return st

    def intensity(self, x, st, scale, shift):
        m = st[:, 0][:, None, None]
        return np.clip(m + (x - m) * scale[:, None, None] + shift[:, None, None], 0, 1).astype(f32)

    def gamma(self, x, st, g):
        a, b = st[:, 1][:, None, None], st[:, 2][:, None, None]
        g = np.asarray(g, dtype=np.float64)[:, None, None]
        if self.fault == "gamma_unnormalised":
            return np.where(b - a > f32(1e-3), (x.astype(np.float64) ** g).astype(f32), x)
        r = np.where(b - a > f32(1e-3), b - a, f32(1))
        t = ((x - a) / r).astype(f32)
        y = np.clip((t.astype(np.float64) ** g).astype(f32) * r + a, a, b).astype(f32)
        return np.where(b - a > f32(1e-3), y, x)

    def impulse(self, x, seed, threshold):
        mask, val = impulses(philox(np.arange(x.size), seed), threshold, word=1 if self.fault == "impulse_wrong_word" else 2)
        return np.where(mask.reshape(x.shape), val.reshape(x.shape), x)

    def smooth(self, x, weights):
        y = x
        for axis in range(3):
            y = scipy.ndimage.correlate1d(y, weights.astype(np.float64), axis=axis, output=f32, mode="mirror" if self.fault == "mirror_border" else "reflect")
        return y

    def defect(self, x, st, mode, contrast_scale):
        if mode is None:
            return x.copy()
        md = mode[:, None, None]
        m = st[:, 0][:, None, None] if st is not None else f32(0)
        return np.where(md == 1, f32(0), np.where(md == 2, f32(1), np.where(md == 3, m + (x - m) * f32(contrast_scale), x))).astype(f32)

    def chain(self, x, plan):
        if self.fault == "defect_before_smooth" and plan.weights is not None:
            import dataclasses
            head = staged(self, x, dataclasses.replace(plan, weights=None, blur=None, defect=None))[-1][2]
            st = self.stats(head) if plan.defect is not None and (plan.defect == 3).any() else None
            return self.smooth(self.defect(head, st, plan.defect, plan.contrast_scale), plan.weights)
        return staged(self, x, plan)[-1][2]


# ---- the cases of tests/test_intensity_gpu.py ----

BLOCKS = {"5x24x24": (5, 24, 24),    # more than one tile row of the smoothing pass
          "3x17x33": (3, 17, 33),    # odd rows, row tails
          "1x20x20": (1, 20, 20),    # the z radius exceeds the axis for every sigma
          "2x7x5": (2, 7, 5)}        # every axis shorter than radius 6: the reflection is repeated
NODES = ("noise", "intensity", "gamma", "impulse", "smooth", "defect")
CASES = [(b, n) for b in BLOCKS for n in ("all",) + NODES + ("smooth05",)]   # smooth05: sigma 0.5, radius 2


def build_block(shape, seed=5):
    """float32 in [0, 1]: random sections, each holding an exact 0 and an exact 1 (range 1: far above gamma's 1e-3); section 1
    constant 0.5 (range 0: gamma's skip branch); section 2 all zero (padding beyond the volume)"""
    rng = np.random.default_rng(seed)
    x = rng.random(shape, dtype=np.float32)
    x[:, 0, 0], x[:, -1, -1] = 0.0, 1.0
    if shape[0] > 1:
        x[1] = 0.5
    if shape[0] > 2:
        x[2] = 0.0
    return x


def build_plan(shape, nodes="all", seed=7):
    """A plan that applies `nodes` ("all" or one name), from its own seeded stream -- the launches are tested on their inputs,
    whatever drew them.  sigma 1.5: radius 6; the gamma exponents include both ends, 0.8 and 1.2, of the default interval;
    the defect modes cycle low contrast, 0, 1, unchanged over the sections; q = 1/2."""
    from bootstrapper_amd.augment import IntensityPlan, gamma_exponent, gamma_interval, gaussian_weights
    rng = np.random.default_rng(seed)
    d = shape[0]
    on = (lambda n: True) if nodes == "all" else (lambda n: n == nodes)
    plan = IntensityPlan(tuple(shape), contrast_scale=0.1, seed=int(rng.integers(0, 2 ** 64, dtype=np.uint64)))
    scale, shift = rng.uniform(0.9, 1.1, d).astype(f32), rng.uniform(-0.1, 0.1, d).astype(f32)
    lo, hi = gamma_interval((0.8, 1.2))
    g = rng.uniform(lo, hi, d)
    g[0] = lo
    g[-1] = hi if d > 1 else lo
    if on("noise"):
        plan.noise_sigma = float(f32(0.1))
    if on("intensity"):
        plan.scale, plan.shift = scale, shift
    if on("gamma"):
        plan.gamma = gamma_exponent(g).astype(f32)
    if on("impulse"):
        plan.impulse_threshold = 2 ** 31
    if on("smooth") or nodes == "smooth05":
        plan.blur = 0.5 if nodes == "smooth05" else 1.5
        plan.weights = gaussian_weights(plan.blur)
    if on("defect"):
        plan.defect = np.array([(3, 1, 2, 0)[z % 4] for z in range(d)], dtype=np.int32)
    return plan
