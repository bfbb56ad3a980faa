"""Reference of ONE launch of the U-Net forward (test infrastructure: numpy / torch float64 on the CPU, no GPU).

tests/test_layers_gpu.py reads every launch's inputs and output back from the device (Model.debug_activation) and
compares the output with a float64 computation of that one operation on the inputs AS THE DEVICE HOLDS THEM;
tests/test_layers_cpu.py runs the same comparison on synthetic stages with emulations (and faulty emulations) of
the kernels' arithmetic in the kernel's place.  This module holds what both share:

  walk()            the planner's list of operations (Planner::run / rec / pass of csrc/unet_plan.hip), from a net config
  Dense / Upsampled tensors that hand out voxels as float64 rows (an upsampled map that the forward never writes is
                    the reference upsampling of the device's low-resolution map, evaluated only where it is read)
  Stage             one conv launch in its GEMM view: out[m, n] = relu(sum_k X[m, k] W[k, n] + b[n]), K = (source, tap,
                    channel) and, for the last stage of a ConvPass, the columns of the cropped 1x1x1 residual branch
  emulations        float64 accumulation of exactly the products a precision mode forms (split-bf16: hi hi + lo hi + hi lo,
                    Winograd F(2x2) / F(4x4) with the matrices of csrc/wino.hip), and the accumulation allowance
  gates             |got - ref| <= g_acc * S + g_out * |ref|,  S = sqrt(conv(x^2, w^2) + b^2)

Why S and not sum |w| |x|: tools/layer_error_scales.py.  Against S the error of a number format is a constant that does
not depend on K, so one gate serves every layer.

g_out (derived, not measured): the unit roundoff of the stored output, every store rounds to nearest even (conv_dev.h:
`(__bf16)v`; no kernel truncates).  f32: 24 significant bits, 2^-24.  bf16: 8 significant bits (7 stored), 2^-8 -- the
value 1 + 2^-8 lies half way between 1 and 1 + 2^-7 and is stored as 1 (tests/test_layers_cpu.py pins this; 2^-9 would refuse
a correctly rounded store, truncation would be 2^-7).  Split: hi = bf16(v) leaves |v - hi| <= 2^-8 2^e, and lo = bf16(v - hi)
is exact when |v - hi| = 2^-8 2^e and otherwise rounds a value below 2^(e-8) to 8 bits: 2^-17.
g_acc = MARGIN * max(e_fmt, e_acc32), both computed here from the reference alone, never from the kernel under test:
e_fmt is the S-normalised error of the emulation of the step's form against float64 on the same inputs, e_acc32 the
larger of (a) torch's CPU f32 conv3d against float64 and (b) a sequential f32 accumulation in the kernel's K order, rounded
once per MFMA instruction (Stage.acc32_sequential).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

MARGIN = 4.0
G_OUT = {"f32": 2.0 ** -24, "bf16x3": 2.0 ** -17, "bf16": 2.0 ** -8}
# what one K-step of the implicit GEMM holds (conv_igemm.h: kUnitsPerStep units of 32 bytes): channels of one tap
KSTEP_CHANNELS = {"f32": 16, "bf16": 32, "bf16x3": 32}
UNIT_CHANNELS = {"f32": 8, "bf16": 16, "bf16x3": 16}
# products that one MFMA instruction adds to its f32 accumulator (conv_dev.h): v_mfma_f32_32x32x2_f32, v_mfma_f32_32x32x16_bf16
# (the 16x16x32 form of some tiles takes 32: fewer roundings)
MFMA_K = {"f32": 2, "bf16": 16, "bf16x3": 16}
CHAN_PAD = 16   # common.h kChanPad
M_TILE = 256    # rows of a GEMM tile (every TileCfg)


# ---- number formats ---------------------------------------------------------------------------------------------------
def bf16_rne(a):
    """float32 -> nearest bf16 (ties to even), returned as float32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(a.shape)


def split_bf16(a):
    """(hi, lo) of the split mode: hi = bf16(v), lo = bf16(v - hi); float64 arrays."""
    a = np.asarray(a, dtype=np.float32)
    hi = bf16_rne(a)
    lo = bf16_rne(a - hi)
    return hi.astype(np.float64), lo.astype(np.float64)


def store(a, prec):
    """A value as the mode stores it (float32 array holding the stored value exactly)."""
    a = np.asarray(a).astype(np.float32)
    if prec == "f32":
        return a
    if prec == "bf16":
        return bf16_rne(a)
    hi = bf16_rne(a)
    return hi + bf16_rne(a - hi)   # exact in f32


# ---- the planner's list of operations -----------------------------------------------------------------------------------
def _lift(k):
    k = [int(v) for v in k]
    return [1] + k if len(k) == 2 else k


def walk(net_config, in_shape):
    """The launches of one forward in the planner's order.  Every entry has `type` and `shape` (D, H, W, C) and
    input   -
    conv    prefix, conv (index inside the ConvPass), kernel, src = [(step, origin, channels)] of the stage's input (the
            ConvPass input for conv 0, the previous stage otherwise), res = the same for the cropped 1x1x1 residual branch
            of the last stage (origins include the centre crop), else None
    pool    src (step), factor
    up      src (step), factor, offset (crop origin inside the upsampled map)
    head    src (step), prefix
    """
    from bootstrapper_amd.unet import HEAD_OF_OUTPUT, input_channels
    dfs = [_lift(f) for f in net_config["downsample_factors"]]
    nl = len(dfs) + 1
    nd = len(net_config["downsample_factors"][0]) if dfs else 3
    k3 = [3] * nd
    ksd = [[_lift(k) for k in ks] for ks in (net_config.get("kernel_size_down") or [[k3, k3]] * nl)]
    ksu = [[_lift(k) for k in ks] for ks in (net_config.get("kernel_size_up") or [[k3, k3]] * (nl - 1))]
    nf, inc = int(net_config["num_fmaps"]), int(net_config["fmap_inc_factor"])
    nf_out = int(net_config.get("num_fmaps_out") or 0)
    fm = [nf * inc ** l for l in range(nl)]
    crop_factor, prod = [None] * (nl - 1), [1, 1, 1]
    for l in range(nl - 2, -1, -1):
        prod = [a * b for a, b in zip(prod, dfs[l])]
        crop_factor[l] = list(prod)
    steps = []

    def add(**kw):
        steps.append(kw)
        return len(steps) - 1

    def conv_pass(prefix, ins, sp, cout, ks):
        crop = [sum(k[d] - 1 for k in ks) for d in range(3)]
        cur = None
        for ci, k in enumerate(ks):
            out_sp = [sp[d] - (k[d] - 1) for d in range(3)]
            if min(out_sp) <= 0:
                raise ValueError(f"{prefix}: input extent {sp} too small for kernel {k}")
            src = list(ins) if ci == 0 else [(cur, (0, 0, 0), cout)]
            res = None
            if ci == len(ks) - 1:
                res = [(s, tuple(o[d] + crop[d] // 2 for d in range(3)), c) for s, o, c in ins]
            cur = add(type="conv", prefix=prefix, conv=ci, kernel=tuple(k), shape=tuple(out_sp) + (cout,), src=src, res=res)
            sp = out_sp
        return cur, sp

    def rec(level, f_in, sp, cin):
        i = nl - level - 1
        f_left, dims = conv_pass(f"unet.l_conv.{i}", [(f_in, (0, 0, 0), cin)], sp, fm[i], ksd[i])
        if level == 0:
            return f_left, dims, fm[i]
        f = dfs[i]
        if any(dims[d] % f[d] for d in range(3)):
            raise ValueError(f"can not downsample {dims} with factor {f}")
        g_sp = [dims[d] // f[d] for d in range(3)]
        g_in = add(type="pool", src=f_left, factor=tuple(f), shape=tuple(g_sp) + (fm[i],))
        g_out, g_dims, g_c = rec(level - 1, g_in, g_sp, fm[i])
        up = [g_dims[d] * f[d] for d in range(3)]
        conv_crop = [sum(k[d] - 1 for k in ksu[i]) for d in range(3)]
        target = [int(math.floor((up[d] - conv_crop[d]) / crop_factor[i][d])) * crop_factor[i][d] + conv_crop[d] for d in range(3)]
        g_c_step = add(type="up", src=g_out, factor=tuple(f), offset=tuple((up[d] - target[d]) // 2 for d in range(3)),
                       shape=tuple(target) + (g_c,))
        so = tuple((dims[d] - target[d]) // 2 for d in range(3))
        cout = nf_out if (i == 0 and nf_out > 0) else fm[i]
        out, out_sp = conv_pass(f"unet.r_conv.0.{i}", [(f_left, so, fm[i]), (g_c_step, (0, 0, 0), g_c)], target, cout, ksu[i])
        return out, out_sp, cout

    cin = input_channels(net_config)
    x = add(type="input", shape=tuple(int(s) for s in in_shape) + (cin,))
    z, z_sp, z_c = rec(nl - 1, x, [int(s) for s in in_shape], cin)
    for name, val in net_config["outputs"].items():
        add(type="head", src=z, prefix=HEAD_OF_OUTPUT[name], shape=tuple(z_sp) + (int(val["dims"]),))
    return steps


def check_walk(ops, plan):
    """The walker against Model.plan_steps(): types, shapes, prefixes and conv indices, step by step."""
    assert len(ops) == len(plan), (len(ops), len(plan))
    for i, (o, p) in enumerate(zip(ops, plan)):
        assert o["type"] == p["type"], (i, o["type"], p["type"])
        assert tuple(o["shape"]) == tuple(p["shape"]), (i, o["type"], o["shape"], p["shape"])
        if o["type"] == "conv":
            assert (o["prefix"], o["conv"]) == (p["prefix"], p["conv"]), (i, o["prefix"], o["conv"], p["prefix"], p["conv"])
        if o["type"] == "head":
            assert o["prefix"] == p["prefix"], (i, o["prefix"], p["prefix"])
        if o["type"] in ("pool", "up"):
            assert tuple(o["factor"]) == tuple(p["factor"]), (i, o["factor"], p["factor"])
        if o["type"] == "up":
            assert tuple(o["offset"]) == tuple(p["offset"]), (i, o["offset"], p["offset"])


# ---- tensors ------------------------------------------------------------------------------------------------------------
class Dense:
    """A (D, H, W, C) array (kept in its own dtype; rows come out as float64)."""

    def __init__(self, a):
        self.a = a
        self.shape = a.shape

    def at(self, z, y, x):
        return self.a[z, y, x].astype(np.float64)

    def full(self):
        return self.a.astype(np.float64)


def _lin_src(dst, f, n):
    """torch's source index rule of linear interpolation, align_corners=False (area_pixel_compute_source_index)."""
    src = np.maximum((dst + 0.5) / f - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    w1 = np.clip(src - i0, 0.0, 1.0)
    return i0, i1, 1.0 - w1, w1


class Upsampled:
    """Trilinear upsampling (align_corners=False) of `low` by `factor`, then the crop at `offset` to `shape`, in float64,
    evaluated at the voxels asked for."""

    def __init__(self, low, factor, offset, shape):
        self.low, self.f, self.o = low, factor, offset
        self.shape = tuple(shape)

    def at(self, z, y, x):
        D, H, W = self.low.shape[:3]
        z0, z1, wz0, wz1 = _lin_src(np.asarray(z) + self.o[0], self.f[0], D)
        y0, y1, wy0, wy1 = _lin_src(np.asarray(y) + self.o[1], self.f[1], H)
        x0, x1, wx0, wx1 = _lin_src(np.asarray(x) + self.o[2], self.f[2], W)
        out = 0.0
        for zi, wz in ((z0, wz0), (z1, wz1)):
            for yi, wy in ((y0, wy0), (y1, wy1)):
                for xi, wx in ((x0, wx0), (x1, wx1)):
                    w = wz * wy * wx
                    if np.any(w != 0):
                        out = out + w[:, None] * self.low.at(zi, yi, xi)
        return out

    def full(self, fn=None, unit_weights=False):
        """The whole map, separably (fn: applied to the low-resolution values first, e.g. np.abs; unit_weights: every neighbour
        with weight 1 -- with fn = np.abs the scale of what an error of the weights themselves can do)."""
        a = self.low.full()
        if fn is not None:
            a = fn(a)
        for d in range(3):
            i0, i1, w0, w1 = _lin_src(np.arange(self.shape[d]) + self.o[d], self.f[d], a.shape[d])
            if unit_weights:
                w0, w1 = np.ones_like(w0), np.ones_like(w1)
            sh = [1, 1, 1, 1]
            sh[d] = -1
            a = np.take(a, i0, axis=d) * w0.reshape(sh) + np.take(a, i1, axis=d) * w1.reshape(sh)
        return a

    def weight_error(self):
        """How far the kernel's f32 interpolation weights may lie from the exact ones.  A factor that is a power of two gives
        weights that f32 holds exactly (1/4, 3/4, ...).  Otherwise the source coordinate (dst + 0.5) * (1 / f) - 0.5, as large as
        the low-resolution extent n, carries the rounding of 1 / f, of the product and of the difference (or of one fma):
        at most 3 * 2^-24 * (n + 1) per axis, and the weights are differences of it."""
        return sum(3 * 2.0 ** -24 * (n + 1) for n, f in zip(self.low.shape[:3], self.f) if f & (f - 1))


def maxpool(a, f):
    D, H, W, C = a.shape
    return a.reshape(D // f[0], f[0], H // f[1], f[1], W // f[2], f[2], C).max(axis=(1, 3, 5))


def all_voxels(shape):
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape[:3]], indexing="ij")
    return z.ravel(), y.ravel(), x.ravel()


# ---- one conv launch in its GEMM view -------------------------------------------------------------------------------------
class Stage:
    """src / res: [(tensor, origin, channels)] as in walk(); w: (Cout, Cin_total, kz, ky, kx), b: (Cout,);
    wr: (Cout, Cin_res_total, 1, 1, 1) and br for the residual branch of a last stage.  Columns of K: for every source, tap
    major, channels inside; then the residual's channels source by source."""

    def __init__(self, src, kernel, w, b, res=None, wr=None, br=None, relu=True):
        self.src, self.kernel, self.res, self.relu = src, tuple(kernel), res, relu
        w = np.asarray(w, dtype=np.float32)
        self.cout = w.shape[0]
        cols, blocks, base = [], [], 0
        taps = [(dz, dy, dx) for dz in range(kernel[0]) for dy in range(kernel[1]) for dx in range(kernel[2])]
        for s, (_, _, c) in enumerate(src):
            for t, (dz, dy, dx) in enumerate(taps):
                blocks.append(w[:, base:base + c, dz, dy, dx].T)
                cols += [(0, s, t, ch) for ch in range(c)]
            base += c
        assert base == w.shape[1], (base, w.shape)
        self.bias = np.asarray(b, dtype=np.float32).astype(np.float64)
        if res is not None:
            wr = np.asarray(wr, dtype=np.float32)
            base = 0
            for s, (_, _, c) in enumerate(res):
                blocks.append(wr[:, base:base + c, 0, 0, 0].T)
                cols += [(1, s, 0, ch) for ch in range(c)]
                base += c
            assert base == wr.shape[1]
            self.bias_res = np.asarray(br, dtype=np.float32).astype(np.float64)
        else:
            self.bias_res = np.zeros(self.cout)
        self.taps = taps
        self.W32 = np.ascontiguousarray(np.concatenate(blocks, axis=0))   # (K, Cout) float32
        self.W = self.W32.astype(np.float64)
        self.cols = np.array(cols, dtype=np.int64)                        # (K, 4): is_res, source, tap, channel
        self.b = self.bias + self.bias_res

    def rows(self, z, y, x, res_shift=(0, 0, 0)):
        """X (n, K) float64 of the output voxels (z, y, x)."""
        parts = []
        for t, o, _ in self.src:
            for dz, dy, dx in self.taps:
                parts.append(t.at(z + o[0] + dz, y + o[1] + dy, x + o[2] + dx))
        for t, o, _ in (self.res or []):
            parts.append(t.at(z + o[0] + res_shift[0], y + o[1] + res_shift[1], x + o[2] + res_shift[2]))
        return np.concatenate(parts, axis=1)

    def act(self, pre):
        return np.maximum(pre, 0.0) if self.relu else pre

    def ref(self, X):
        """(pre-activation in float64, S)."""
        pre = X @ self.W + self.b
        S = np.sqrt((X * X) @ (self.W * self.W) + self.bias ** 2 + self.bias_res ** 2)
        return pre, S

    # -- emulations of the direct forms: float64 accumulation of the products the mode forms ------------------------------
    def emulate(self, X, prec, fault=None, part="all"):
        """Pre-activation sums of the direct (non-Winograd) kernels of `prec` on the rows X (values as the device holds them).
        fault: None, ("lo_tap", tap), ("kstep", tap), ("bias", channel) -- see tests/test_layers_cpu.py.
        part="res": the residual branch alone, with its own bias (what a Winograd stage adds to its transform's sums)."""
        W, b = self.W, self.b.copy()
        if part == "res":
            X = X * (self.cols[:, 0] == 1)
            b = self.bias_res.copy()
        if fault and fault[0] == "kstep":      # one 32-channel K-step of one tap of the first source never accumulated
            X = X.copy()
            c = self.cols
            X[:, (c[:, 0] == 0) & (c[:, 1] == 0) & (c[:, 2] == fault[1]) & (c[:, 3] < 32)] = 0.0
        if fault and fault[0] == "bias":
            b[fault[1]] = 0.0
        if prec == "f32":
            return X @ W + b
        if prec == "bf16":
            return X @ bf16_rne(self.W32).astype(np.float64) + b
        Wh, Wl = split_bf16(self.W32)
        if fault and fault[0] == "lo_tap":     # the lo part of the weights of one tap lost
            c = self.cols
            Wl = Wl.copy()
            Wl[(c[:, 0] == 0) & (c[:, 1] == 0) & (c[:, 2] == fault[1])] = 0.0
        Xh = bf16_rne(X.astype(np.float32)).astype(np.float64)
        return X @ Wh + Xh @ Wl + b            # (hi + lo) hi + hi lo

    # -- the accumulation allowance ---------------------------------------------------------------------------------------
    def ksteps(self, prec, wino=False):
        """Column indices of K, K-step by K-step, in the order the kernel walks them (build_entries of unet_pack.hip: per
        source, chunks of one K-step's channels with the taps inside -- a source of at most one unit's channels pairs two
        x-adjacent taps per K-step --, then the residual's chunks; Winograd (wino_units): per 32-channel chunk the three z
        taps, a K-step being the in-plane taps of one z tap in the transform domain)."""
        kc, unit = KSTEP_CHANNELS[prec], UNIT_CHANNELS[prec]
        c = self.cols
        kz, ky, kx = self.kernel
        tz, ty, tx = c[:, 2] // (ky * kx), (c[:, 2] // kx) % ky, c[:, 2] % kx
        nch = np.array([s[2] for s in self.src] + [0])
        narrow = (-(-nch[c[:, 1]] // CHAN_PAD) * CHAN_PAD == unit) & (c[:, 0] == 0)
        if wino:
            key = np.stack([c[:, 0], c[:, 1], c[:, 3] // 32, np.where(c[:, 0] == 0, tz, 0), 0 * tz, 0 * tz], axis=1)
        else:
            key = np.stack([c[:, 0], c[:, 1], np.where(narrow, 0, c[:, 3] // kc), tz, ty, np.where(narrow, tx // 2, tx)], axis=1)
        order = np.lexsort(key.T[::-1])
        ks = key[order]
        cut = np.flatnonzero(np.any(ks[1:] != ks[:-1], axis=1)) + 1
        return np.split(order, cut)

    def acc32_sequential(self, X, prec, wino=False, split_k=False, max_rows=512, max_cols=64, seed=0):
        """(sums, pre, S) on a seeded subset of at most max_rows rows and max_cols output channels: the sum as the matrix pipe
        forms it -- the products of ONE MFMA instruction (MFMA_K: 2 in f32, 16 in the bf16 modes) added in float64, the
        instructions of a K-step and the K-steps one after the other in float32; split_k: the sum cut in two halves that are
        added last -- next to the float64 sums and S of the same elements.
        (The first form of this allowance rounded once per K-step.  The full net's second 60-channel stage in f32 then sat at
        5.5e-6 of S against a gate of 5.2e-6: the f32 MFMA rounds its accumulator every 2 products, 816 times in that stage, not
        110 times.  The arithmetic is stated here as the instruction performs it; the margin stays 4.)"""
        rng = np.random.default_rng(seed)
        rows = np.sort(rng.choice(X.shape[0], max_rows, replace=False)) if X.shape[0] > max_rows else np.arange(X.shape[0])
        cols = np.sort(rng.choice(self.cout, max_cols, replace=False)) if self.cout > max_cols else np.arange(self.cout)
        steps = self.ksteps(prec, wino)
        g = MFMA_K[prec]
        order = np.concatenate(steps)
        bounds, pos = [], 0
        for idx in steps:
            bounds += [(pos + j, min(pos + j + g, pos + len(idx))) for j in range(0, len(idx), g)]
            pos += len(idx)
        Xo = np.ascontiguousarray(X[rows][:, order])
        Wo = np.ascontiguousarray(self.W[order][:, cols])
        halves = [bounds[:len(bounds) // 2], bounds[len(bounds) // 2:]] if (split_k and len(bounds) > 1) else [bounds]
        total = None
        for part in halves:
            acc = np.zeros((len(rows), len(cols)), dtype=np.float32)
            for a, b in part:
                acc += (Xo[:, a:b] @ Wo[a:b]).astype(np.float32)
            total = acc if total is None else total + acc
        b = self.b[cols]
        sums = (total + b.astype(np.float32)).astype(np.float64)
        pre = Xo @ Wo + b
        S = np.sqrt((Xo * Xo) @ (Wo * Wo) + self.bias[cols] ** 2 + self.bias_res[cols] ** 2)
        return sums, pre, S

    def acc32_torch(self, X):
        """f32 GEMM of torch's CPU backend on the same rows (what stands in for its f32 conv3d where only sampled rows exist)."""
        r = torch.from_numpy(X.astype(np.float32)) @ torch.from_numpy(self.W32) + torch.from_numpy(self.b.astype(np.float32))
        return r.numpy().astype(np.float64)


def conv3d_f32(stage, shape):
    """torch's CPU f32 conv3d (the arithmetic of oracle/unet_ref.py) of a whole stage: pre-activation (D, H, W, Cout)."""
    Do, Ho, Wo = shape[:3]
    kz, ky, kx = stage.kernel

    def block(srcs, ext):
        parts = []
        for t, o, _ in srcs:
            a = t.full() if not isinstance(t, Dense) else t.a
            parts.append(np.asarray(a[o[0]:o[0] + ext[0], o[1]:o[1] + ext[1], o[2]:o[2] + ext[2]], dtype=np.float32))
        return torch.from_numpy(np.ascontiguousarray(np.concatenate(parts, axis=3).transpose(3, 0, 1, 2)))[None]

    nmain = int((stage.cols[:, 0] == 0).sum())
    cin = nmain // (kz * ky * kx)
    # W32 rows are (source, tap, channel): back to (Cout, Cin, kz, ky, kx)
    w, base, row = [], 0, 0
    for _, _, c in stage.src:
        blk = stage.W32[row:row + kz * ky * kx * c].reshape(kz, ky, kx, c, stage.cout)
        w.append(blk.transpose(4, 3, 0, 1, 2))
        row += kz * ky * kx * c
        base += c
    w = torch.from_numpy(np.ascontiguousarray(np.concatenate(w, axis=1)))
    assert w.shape[1] == cin
    with torch.no_grad():
        out = F.conv3d(block(stage.src, (Do + kz - 1, Ho + ky - 1, Wo + kx - 1)), w, torch.from_numpy(stage.bias.astype(np.float32)))
        if stage.res is not None:
            wr = torch.from_numpy(np.ascontiguousarray(stage.W32[nmain:].T))[:, :, None, None, None]
            out = out + F.conv3d(block(stage.res, (Do, Ho, Wo)), wr, torch.from_numpy(stage.bias_res.astype(np.float32)))
    return out[0].numpy().transpose(1, 2, 3, 0).astype(np.float64)


# ---- Winograd F(m x m, 3 x 3) in (y, x), split-bf16 operands (csrc/wino.hip) -------------------------------------------------
_R2 = math.sqrt(2.0)
WINO = {
    2: dict(BT=np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64),
            G=np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64),
            AT=np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)),
    # interpolation points 0, +-1/sqrt2, +-sqrt2, inf
    4: dict(BT=np.array([[1, 0, -2.5, 0, 1, 0], [0, _R2, 2, -_R2 / 2, -1, 0], [0, -_R2, 2, _R2 / 2, -1, 0],
                         [0, -_R2, -1, 2 * _R2, 2, 0], [0, _R2, -1, -2 * _R2, 2, 0], [0, 1, 0, -2.5, 0, 1]], dtype=np.float64),
            G=np.array([[1, 0, 0], [2 / 3, 2 / 3 / _R2, 1 / 3], [2 / 3, -2 / 3 / _R2, 1 / 3], [1 / 12, _R2 / 12, 1 / 6],
                        [1 / 12, -_R2 / 12, 1 / 6], [0, 0, 1]], dtype=np.float64),
            AT=np.array([[1, 1, 1, 1, 1, 0], [0, 1 / _R2, -1 / _R2, _R2, -_R2, 0], [0, .5, .5, 2, 2, 0],
                         [0, _R2 ** -3, -_R2 ** -3, _R2 ** 3, -_R2 ** 3, 1]], dtype=np.float64)),
}


def wino_emulate(x, w, m, clamp_rows=0):
    """Sums of a valid 3x3x3 convolution (no bias) in the Winograd form of the split mode.  x: (D, H, W, C) float32 values as
    the device holds them (hi + lo), w: (Cout, C, 3, 3, 3) float32.  V = B^T d B in f32 and U = G g G^T (made in double,
    rounded to f32, as wino_pack_weights does) are both stored as (hi, lo) pairs; M = sum over (kz, c) of Vhi Uhi + Vlo Uhi
    + Vhi Ulo, accumulated in float64 here; A^T M A in f32.  The last tile row / column of an extent that is no multiple of m
    overhangs: its reads are clamped to the input and the outputs that depend on them are cut.
    clamp_rows (fault injection): the clamp sets in that many rows too early."""
    mats = WINO[m]
    T = m + 2
    x = np.asarray(x, dtype=np.float32)
    D, H, W, C = x.shape
    Do, Ho, Wo = D - 2, H - 2, W - 2
    Ty, Tx = -(-Ho // m), -(-Wo // m)
    yi = np.minimum(np.arange(Ty * m + 2), H - 1 - clamp_rows)
    xi = np.minimum(np.arange(Tx * m + 2), W - 1)
    xp = x[:, yi][:, :, xi]
    ty = (np.arange(Ty) * m)[:, None] + np.arange(T)[None]      # (Ty, T)
    tx = (np.arange(Tx) * m)[:, None] + np.arange(T)[None]
    d = xp[:, ty][:, :, :, tx]                                  # (D, Ty, T, Tx, T, C)
    BT = mats["BT"].astype(np.float32)
    V = np.einsum("ai,zpiqjc,bj->abzpqc", BT, d, BT, optimize=True).astype(np.float32)
    Vh, Vl = split_bf16(V)
    g = np.asarray(w, dtype=np.float32).astype(np.float64)      # (N, C, kz, ky, kx)
    U = np.einsum("ay,nczyx,bx->abzcn", mats["G"], g, mats["G"], optimize=True).astype(np.float32)
    Uh, Ul = split_bf16(U)
    Vs = Vh + Vl
    N = w.shape[0]
    Mx = np.zeros((T, T, Do * Ty * Tx, N))
    for kz in range(3):
        Mx += np.matmul(Vs[:, :, kz:kz + Do].reshape(T, T, -1, C), Uh[:, :, kz])
        Mx += np.matmul(Vh[:, :, kz:kz + Do].reshape(T, T, -1, C), Ul[:, :, kz])
    Mx = Mx.reshape(T, T, Do, Ty, Tx, N)
    AT = mats["AT"].astype(np.float32)
    Y = np.einsum("ua,abzpqn,vb->zpuqvn", AT, Mx.astype(np.float32), AT, optimize=True).astype(np.float32)
    return Y.reshape(Do, Ty * m, Tx * m, -1)[:, :Ho, :Wo].astype(np.float64)


# ---- the comparison ------------------------------------------------------------------------------------------------------
def gate(e_fmt, e_acc32):
    return MARGIN * max(e_fmt, e_acc32)


def allowances(stage, X, pre, S, prec, wino=False, split_k=False, emu_pre=None, f32_pre=None):
    """(e_fmt, e_acc32) of a stage on the rows X: the S-normalised error against float64 of the emulation of the step's form
    (emu_pre: the Winograd emulation's sums on the same rows; default the direct form of `prec`), and the larger of the errors
    of torch's CPU f32 arithmetic (f32_pre: its conv3d on these rows; default its GEMM) and of the sequential f32 K-step sum."""
    e_fmt = norm_err(stage.emulate(X, prec) if emu_pre is None else emu_pre, pre, S)
    e_seq = norm_err(*stage.acc32_sequential(X, prec, wino, split_k))
    e_blas = norm_err(stage.acc32_torch(X) if f32_pre is None else f32_pre, pre, S)
    return e_fmt, max(e_seq, e_blas)


def norm_err(a, pre, S):
    """Largest |a - pre| / S (S = 0 only where every product and the bias are zero: then a must equal pre)."""
    d = np.abs(a - pre)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(S > 0, d / S, np.where(d > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def compare(got, ref, S, g_acc, g_out):
    """|got - ref| <= g_acc S + g_out |ref| element-wise, arrays of (n, C).  Returns (ok, worst) with worst = dict of the element
    that exceeds its bound by the largest factor (row, channel, err, S, err / S, bound) and the largest err / S overall."""
    err = np.abs(got - ref)
    bound = g_acc * S + g_out * np.abs(ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
        es = np.where(S > 0, err / S, 0.0)
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    r, c = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    worst = dict(row=int(r), channel=int(c), err=float(err[r, c]), S=float(S[r, c]), err_over_S=float(es[r, c]),
                 bound=float(bound[r, c]), ref=float(ref[r, c]), got=float(got[r, c]), max_err_over_S=float(es.max()))
    return bool(ratio[r, c] <= 1.0), worst


def describe(worst, vox, shape):
    """Where the worst element is: voxel, channel, its GEMM tile and row."""
    z, y, x = (int(v[worst["row"]]) for v in vox)
    flat = (z * shape[1] + y) * shape[2] + x
    return (f"(z, y, x, c) = ({z}, {y}, {x}, {worst['channel']}), M-tile {flat // M_TILE} row {flat % M_TILE}: got {worst['got']:.9g} "
            f"ref {worst['ref']:.9g} err {worst['err']:.3e} S {worst['S']:.3e} err/S {worst['err_over_S']:.3e} bound {worst['bound']:.3e}")


def sample_voxels(shape, n_random, rng, wino_m=0, tile_stride=64, min_total=4096):
    """The voxels a sampled check of a (D, H, W) output must contain: the 8 corners, the last flat index, the rows on both sides of
    every M-tile boundary in a stride of at most `tile_stride` tiles, a full row of voxels through the last tile row and one
    through the last tile column of a Winograd stage, and n_random uniformly random ones; at least min_total in all."""
    D, H, W = shape[:3]
    M = D * H * W
    idx = [z * H * W + y * W + x for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)] + [M - 1]
    ntiles = -(-M // M_TILE)
    for t in list(range(1, ntiles, tile_stride)) + [ntiles - 1]:
        if 0 < t < ntiles:
            idx += [t * M_TILE - 1, min(t * M_TILE, M - 1)]
    if wino_m:
        zc = D // 2
        idx += [(zc * H + (H - 1)) * W + x for x in range(W)]          # through the last tile row
        idx += [(zc * H + y) * W + (W - 1) for y in range(H)]          # through the last tile column
    idx += list(rng.integers(0, M, size=n_random))
    idx = np.unique(np.array(idx, dtype=np.int64))
    if len(idx) < min(min_total, M):   # (duplicates among the random ones, few tiles)
        rest = np.setdiff1d(np.arange(M) if M <= 4 * min_total else rng.integers(0, M, size=4 * min_total), idx)
        idx = np.unique(np.concatenate([idx, rng.permutation(rest)[:min(min_total, M) - len(idx)]]))
    return idx // (H * W), (idx // W) % H, idx % W
