"""The batched intensity chain of the 2-D setups (bootstrapper_amd/augment2d.py, csrc/augment2d_intensity.hip, DESIGN.md
section 7m) against tests/intensity_ref.py, which holds every rule, gate and float64 comparison: nothing numerical is added here.
The reference for a batch (K, S, H, W) is intensity_ref's rules applied to each draw's stack x[:, s] with that draw's plan.

Here are the cases, the comparisons shared by the GPU test (on the device) and the CPU test (on the emulation below), and a
float32 emulation of the batched launches that reads the PACKED tables -- the descriptors, the per-plane tables, the taps --
as the kernels do, node by node through intensity_ref.Emulation, into which the CPU test injects indexing faults.

A backend `nodes` runs one batched launch each on a numpy float32 batch and returns the new batch: noise(b), impulse(b),
smooth(b), stats(b) -> (K * S, 3), intensity(b, stats), gamma(b, stats), defect(b, stats, final_map), chain(b, final_map)."""
import numpy as np
import scipy.ndimage

import intensity_ref as R

f32 = np.float32
CASES = {   # S, K, section (H, W), the third draw's plan
    "S3_K3_24x24": (3, 3, (24, 24), "smooth05"),
    "S3_K3_17x33": (3, 3, (17, 33), "noise"),
    "S3_K1_20x20": (3, 1, (20, 20), "gamma"),        # the z radius exceeds the axis
    "S2_K2_7x5": (2, 2, (7, 5), None),               # every axis shorter than radius 6
}
FAULTS = ("previous_descriptor", "plane_transposed", "batch_linear_counter", "z_stride_of_one_plane", "taps_of_draw_0", "final_map_on_untouched")


def build_case(case):
    """(x float32 (K, S, H, W), plans): draw 0 applies every node (sigma 1.5, missing and low-contrast sections), draw 1 is
    untouched, draw 2 (where S = 3) is smooth-only with sigma 0.5 or one other node; every draw from its own seeds, so that a
    draw reading another's descriptor, row or taps shows.  The stacks are intensity_ref.build_block's: a constant section, an
    all-zero section, sections of range 1."""
    from bootstrapper_amd.augment import IntensityPlan
    S, K, (H, W), third = CASES[case]
    shape = (K, H, W)
    plans = [R.build_plan(shape, "all", seed=7), IntensityPlan(shape)] + ([R.build_plan(shape, third, seed=9)] if S == 3 else [])
    x = np.stack([R.build_block(shape, seed=5 + s) for s in range(S)], axis=1)
    return np.ascontiguousarray(x), plans


# ---- the comparisons ----

class DrawOps:
    """The backend intensity_ref.staged wants, for draw s of a batch: the stack under test is put in as draw s of `batch`, the
    BATCHED launch runs on all draws, and draw s is read back.  The node's numbers come from the packed tables, not from the
    arguments staged passes (they are the plan's, which the tables were made of)."""

    def __init__(self, nodes, s, batch):
        self.nodes, self.s, self.batch = nodes, s, batch
        self.K, self.S = batch.shape[:2]

    def _put(self, x):
        b = self.batch.copy()
        b[:, self.s] = x
        return b

    def _stats(self, b, st):
        full = self.nodes.stats(b)
        if st is not None:
            full.reshape(self.K, self.S, 3)[:, self.s] = st
        return full

    def stats(self, x):
        return self.nodes.stats(self._put(x)).reshape(self.K, self.S, 3)[:, self.s].copy()

    def noise(self, x, seed, sigma):
        return self.nodes.noise(self._put(x))[:, self.s].copy()

    def impulse(self, x, seed, threshold):
        return self.nodes.impulse(self._put(x))[:, self.s].copy()

    def smooth(self, x, weights):
        return self.nodes.smooth(self._put(x))[:, self.s].copy()

    def intensity(self, x, st, scale, shift):
        b = self._put(x)
        return self.nodes.intensity(b, self._stats(b, st))[:, self.s].copy()

    def gamma(self, x, st, g):
        b = self._put(x)
        return self.nodes.gamma(b, self._stats(b, st))[:, self.s].copy()

    def defect(self, x, st, mode, contrast_scale):
        b = self._put(x)
        return self.nodes.defect(b, self._stats(b, st), False)[:, self.s].copy()


def compare(nodes, x, plans, block, show=print):
    """Every comparison of one case; raises AssertionError naming the draw and the node.  `block`: the 3-D chain the batched one
    must equal bit for bit -- block.chain(stack, plan, final_map) and block.node(name, stack, plan, stats (K, 3)) -> stack."""
    K, S = x.shape[:2]
    final, plain = nodes.chain(x, True), nodes.chain(x, False)
    assert np.array_equal(nodes.chain(x, True), final), "two runs of one packed plan differ"
    # 1, 2: every touched draw is the 3-D chain of its own stack, bit for bit; an untouched draw is its input
    for s, plan in enumerate(plans):
        stack = np.ascontiguousarray(x[:, s])
        if plan.applied:
            assert np.array_equal(final[:, s], block.chain(stack, plan, True)), f"draw {s}: the batched chain differs from the 3-D chain of its stack"
            assert np.array_equal(plain[:, s], block.chain(stack, plan, False)), f"draw {s}: the batched chain before the final map differs"
            assert final[:, s].min() >= -1.0 and final[:, s].max() <= 1.0
        else:
            assert np.array_equal(final[:, s], stack) and np.array_equal(plain[:, s], stack), f"draw {s}: an untouched draw changed"
    # ... and so is every single node, run alone through its own entry
    st = nodes.stats(x)
    for name in R.NODES:
        out = getattr(nodes, name)(x, *(() if name in ("noise", "impulse", "smooth") else (st,) if name != "defect" else (st, False)))
        for s, plan in enumerate(plans):
            stack = np.ascontiguousarray(x[:, s])
            has = {"noise": plan.noise_sigma, "intensity": plan.scale, "gamma": plan.gamma, "impulse": plan.impulse_threshold,
                   "smooth": plan.weights, "defect": plan.defect}[name] is not None
            want = block.node(name, stack, plan, np.ascontiguousarray(st.reshape(K, S, 3)[:, s])) if has else stack
            assert np.array_equal(out[:, s], want), f"draw {s}, {name} alone: " + ("differs from the 3-D launch" if has else "a draw without the node changed")
    # 4: end to end against float64, launch by launch, with intensity_ref's gates
    for s, plan in enumerate(plans):
        if plan.applied:
            stack = np.ascontiguousarray(x[:, s])
            R.check(R.staged(DrawOps(nodes, s, x), stack, plan), plan, plain[:, s], show=lambda line: show(f"draw {s}: {line}"))


class EmulatedBlock:
    """`block` of compare for the CPU test: intensity_ref's float32 emulation of the 3-D launches"""

    def __init__(self):
        self.ops = R.Emulation()

    def chain(self, stack, plan, final_map):
        y = self.ops.chain(stack, plan)
        return f32(2) * y - f32(1) if final_map else y

    def node(self, name, stack, plan, st):
        o = self.ops
        return {"noise": lambda: o.noise(stack, plan.seed, plan.noise_sigma), "intensity": lambda: o.intensity(stack, st, plan.scale, plan.shift),
                "gamma": lambda: o.gamma(stack, st, plan.gamma), "impulse": lambda: o.impulse(stack, plan.seed, plan.impulse_threshold),
                "smooth": lambda: o.smooth(stack, plan.weights), "defect": lambda: o.defect(stack, st, plan.defect, plan.contrast_scale)}[name]()


# ---- a float32 emulation of the batched launches reading the packed tables, with faults to inject ----

NOISE, INTENSITY, GAMMA, IMPULSE, SMOOTH, DEFECT, TOUCHED = 1, 2, 4, 8, 16, 32, 64


class Emulated:
    """The launches of csrc/augment2d_intensity.hip on a batch (K, S, H, W): per plane p = k S + s the draw's descriptor is read
    from the table, the plane's numbers from row p of the per-plane tables, the taps at the descriptor's offset; the arithmetic
    of a node is intensity_ref.Emulation's.  fault (one of FAULTS):
      previous_descriptor     draw s > 0 reads draw s - 1's descriptor
      plane_transposed        the per-plane tables and statistics are read at s K + k
      batch_linear_counter    the Philox counter is the voxel's index in the batch, not in the draw's stack
      z_stride_of_one_plane   the z pass of smoothing walks neighbouring planes of the batch, so it reflects into other draws
      taps_of_draw_0          every smoothed draw filters with draw 0's taps
      final_map_on_untouched  2 x - 1 on every draw"""

    def __init__(self, ipacked, fault=None):
        assert fault is None or fault in FAULTS
        self.t, self.fault, self.ops = ipacked, fault, R.Emulation()
        self.S, self.K = ipacked.S, ipacked.K

    def _desc(self, s):
        return self.t.idraws[max(s - 1, 0) if self.fault == "previous_descriptor" else s]

    def _rows(self, table, s):
        """the K entries of draw s in a per-plane table (last axis K * S or leading axis K * S)"""
        p = [s * self.K + k if self.fault == "plane_transposed" else k * self.S + s for k in range(self.K)]
        return table[p]

    def _counter(self, b, s):
        K, S, H, W = b.shape
        k, i = np.meshgrid(np.arange(K), np.arange(H * W), indexing="ij")
        return ((k * S + s) * H * W + i if self.fault == "batch_linear_counter" else k * H * W + i).ravel()

    def stats(self, b):
        return self.ops.stats(b.reshape((-1,) + b.shape[2:]))

    def noise(self, b):
        out = b.copy()
        for s in range(self.S):
            d = self._desc(s)
            if d.nodes & NOISE:
                n = R.normals(R.philox(self._counter(b, s), d.seed)).reshape(b[:, s].shape).astype(f32)
                out[:, s] = np.clip(b[:, s] + f32(d.noise_sigma) * n, 0, 1).astype(f32)
        return out

    def impulse(self, b):
        out = b.copy()
        for s in range(self.S):
            d = self._desc(s)
            if d.nodes & IMPULSE:
                mask, val = R.impulses(R.philox(self._counter(b, s), d.seed), d.impulse_threshold)
                out[:, s] = np.where(mask.reshape(b[:, s].shape), val.reshape(b[:, s].shape), b[:, s])
        return out

    def intensity(self, b, st):
        out, fl = b.copy(), self.t.planes.view(f32)
        for s in range(self.S):
            if self._desc(s).nodes & INTENSITY:
                out[:, s] = self.ops.intensity(b[:, s], self._rows(st, s), self._rows(fl[0], s), self._rows(fl[1], s))
        return out

    def gamma(self, b, st):
        out, fl = b.copy(), self.t.planes.view(f32)
        for s in range(self.S):
            if self._desc(s).nodes & GAMMA:
                out[:, s] = self.ops.gamma(b[:, s], self._rows(st, s), self._rows(fl[2], s))
        return out

    def smooth(self, b):
        out = b.copy()
        planes = b.reshape((-1,) + b.shape[2:])
        for s in range(self.S):
            d = self._desc(s)
            if not d.nodes & SMOOTH:
                continue
            t = self.t.idraws[0] if self.fault == "taps_of_draw_0" else d
            w = self.t.taps[t.taps_offset:t.taps_offset + 2 * t.radius + 1]
            if self.fault == "z_stride_of_one_plane":
                y = scipy.ndimage.correlate1d(planes, w.astype(np.float64), axis=0, output=f32, mode="reflect").reshape(b.shape)[:, s]
                for axis in (1, 2):
                    y = scipy.ndimage.correlate1d(y, w.astype(np.float64), axis=axis, output=f32, mode="reflect")
                out[:, s] = y
            else:
                out[:, s] = self.ops.smooth(b[:, s], w)
        return out

    def defect(self, b, st, final_map):
        out = b.copy()
        for s in range(self.S):
            d = self._desc(s)
            y = b[:, s]
            if d.nodes & DEFECT:
                y = self.ops.defect(y, self._rows(st, s) if st is not None else None, self._rows(self.t.planes[3], s), d.contrast_scale)
            if final_map and (d.nodes & TOUCHED or self.fault == "final_map_on_untouched"):
                y = f32(2) * y - f32(1)
            out[:, s] = y
        return out

    def chain(self, b, final_map):
        """augment2d.apply_intensity2d's order"""
        n = self.t.nodes
        if n & NOISE:
            b = self.noise(b)
        if n & INTENSITY:
            b = self.intensity(b, self.stats(b))
        if n & GAMMA:
            b = self.gamma(b, self.stats(b))
        if n & IMPULSE:
            b = self.impulse(b)
        if n & SMOOTH:
            b = self.smooth(b)
        return self.defect(b, self.stats(b) if self.t.low_contrast else None, final_map)
