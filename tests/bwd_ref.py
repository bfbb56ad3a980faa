"""Reference of ONE operation of the U-Net backward pass (test infrastructure: numpy / torch float64 on the CPU, no GPU).

tests/test_backward_gpu.py reads, after one Trainer.forward_backward, every gradient tensor back from the device
(Trainer.debug_tensor) and compares it with a float64 computation of that one operation on its inputs AS THE DEVICE HOLDS
THEM; tests/test_backward_cpu.py chains the same operations over a small net against torch's float64 autograd and puts
emulations (and faulty emulations) of the kernels' arithmetic in the kernel's place.  This module holds what both share.
It builds on tests/layer_ref.py (walk, Stage, split_bf16, compare, norm_err, MARGIN, G_OUT).

Tensors are channels-last (D, H, W, C) arrays; weights are OIDHW.  The operations of csrc/train_bwd.hip, train_wgrad.hip and train_plan.hip:

  masked gradient   g = dY [Y > 0] in the interior of a zero tensor with border P (border_of)
  weight gradient   dW[n, c, tap] = sum over output voxels m of g[m, n] x[m + tap, c], per source slot (columns cbase ..) and
                    for the cropped 1x1x1 residual branch of a pass's last stage
  bias gradient     db[n] = sum_m g[m, n]
  input gradient    the transposed convolution: dX[v, c] = sum_tap sum_n gpad[v + tap, n] w[n, c, mirrored tap]; for a pass's
                    first stage plus the residual's columns, read from the LAST stage's padded gradient at the crop offset.
                    In its GEMM view this is a layer_ref.Stage over the padded gradients (dgrad_stage), so the emulations, the
                    K-step order and the accumulation allowance of the forward suite serve it unchanged
  scatter           the concat-input gradient's channel groups added into the crop regions of the skip and the upsampled map
  max-pool          the gradient of a window goes to its FIRST maximum in (z, y, x) scan order (torch: strict >); after a ReLU
                    whole windows of zeros are the common tie
  upsampling        transposed trilinear interpolation (align_corners=False, the upper neighbour clamped at the far edge, the
                    source coordinate clamped at 0) of the cropped map
  head              p = sigmoid((Wc + Wr) z + bc + br): dlogit = dp p (1 - p), dz = (Wc + Wr)^T dlogit, dWc = dWr = dlogit z^T,
                    dbc = dbr = sum dlogit
  WeightedMSELoss   mean of w (p - t)^2 over w > 0 -- over ALL elements when every weighted error is zero -- and dL/dp
  Adam              torch.optim.Adam without weight decay

Gates.  Weight, bias, head-weight and input gradients: |got - ref| <= g_acc S + g_out |ref| with S = sqrt(sum a^2 b^2) and
g_acc = MARGIN max(e_fmt, e_acc32), both from the reference alone: e_fmt the S-normalised error of the emulation of the
launch's products (exact f32: 0; split-bf16: hi hi + lo hi + hi lo), e_acc32 the larger error of (a) a sequential f32
accumulation in the launch's own order -- weight gradients: per line range the products of one MFMA instruction added in
float64 and rounded, instruction after instruction in f32, then the range sums added in f32 in four orders (ascending,
descending, two seeded shuffles: float atomics order them by chance), the largest taken; bias and head-weight sums, which the
kernels reduce per thread, per workgroup and then with float atomics: reduction_allowance -- and (b) torch's CPU f32 product.
"""
import math

import numpy as np
import torch

import layer_ref as L

U = 2.0 ** -24          # unit roundoff of f32
WGRAD_SAMPLE = 2048     # output elements on which a weight-gradient launch's allowances are computed


# ---- geometry -------------------------------------------------------------------------------------------------------------
def pass_crop(kernels):
    return tuple(sum(k[d] - 1 for k in kernels) for d in range(3))


def border_of(kernels, ci):
    """Border of the padded masked gradient of stage ci of a ConvPass: k - 1 for the transposed convolution; the last stage's is
    also read by the residual's columns at the crop offset, crop / 2 before its first voxel."""
    k = kernels[ci]
    if ci == len(kernels) - 1:
        c = pass_crop(kernels)
        return tuple(max(k[d] - 1, c[d] // 2) for d in range(3))
    return tuple(k[d] - 1 for d in range(3))


def pass_kernels(ops, i):
    """kernels of every stage of the ConvPass that conv step i belongs to, and the step index of its stage 0"""
    first = i - ops[i]["conv"]
    ks, j = [], first
    while j < len(ops) and ops[j]["type"] == "conv" and ops[j]["prefix"] == ops[i]["prefix"] and ops[j]["conv"] == j - first:
        ks.append(ops[j]["kernel"])
        j += 1
    return ks, first


def consumers(ops):
    """step -> [(consumer step, kind, slot)] with kind conv (a later stage of the same pass), cat (stage 0 of a pass, through
    the crop / concat), pool, up, head"""
    out = {i: [] for i in range(len(ops))}
    for i, o in enumerate(ops):
        if o["type"] == "conv":
            for sl, (s, _, _) in enumerate(o["src"]):
                out[s].append((i, "conv" if o["conv"] > 0 else "cat", sl))
        elif o["type"] in ("pool", "up", "head"):
            out[o["src"]].append((i, o["type"], 0))
    return out


# ---- elementwise and routing operations -----------------------------------------------------------------------------------------
def masked_gradient(dy, y, P):
    """g = dY [Y > 0] into a zero border; keeps dy's dtype (float32 in: the bits the kernel must produce)."""
    D, H, W, C = dy.shape
    out = np.zeros((D + 2 * P[0], H + 2 * P[1], W + 2 * P[2], C), dtype=dy.dtype)
    out[P[0]:P[0] + D, P[1]:P[1] + H, P[2]:P[2] + W] = np.where(y > 0, dy, np.zeros((), dtype=dy.dtype))
    return out


def interior(gp, P):
    return gp[P[0]:gp.shape[0] - P[0], P[1]:gp.shape[1] - P[1], P[2]:gp.shape[2] - P[2]]


def border_nonzero(gp, P):
    m = np.ones(gp.shape[:3], dtype=bool)
    m[P[0]:gp.shape[0] - P[0], P[1]:gp.shape[1] - P[1], P[2]:gp.shape[2] - P[2]] = False
    return int(np.count_nonzero(gp[m]))


def crop(a, origin, ext):
    return a[origin[0]:origin[0] + ext[0], origin[1]:origin[1] + ext[1], origin[2]:origin[2] + ext[2]]


def scatter(dcat, slots, shapes):
    """The gradient of crop + concat: per slot (origin, channels) an array of `shapes[slot]` that holds the slot's channel group
    of dcat in its crop region and zeros elsewhere (dtype kept: a copy, bit for bit)."""
    out, c0 = [], 0
    for (org, c), shp in zip(slots, shapes):
        a = np.zeros(tuple(shp[:3]) + (c,), dtype=dcat.dtype)
        a[org[0]:org[0] + dcat.shape[0], org[1]:org[1] + dcat.shape[1], org[2]:org[2] + dcat.shape[2]] = dcat[..., c0:c0 + c]
        out.append(a)
        c0 += c
    return out


def maxpool_backward(x, dout, f, last=False):
    """din of a max-pool with window = stride = f: the window's gradient at its first maximum in (z, y, x) scan order (numpy's
    argmax returns the first).  last (fault injection): at the last one."""
    D, H, W, C = x.shape
    Do, Ho, Wo = D // f[0], H // f[1], W // f[2]
    win = x.reshape(Do, f[0], Ho, f[1], Wo, f[2], C).transpose(0, 2, 4, 6, 1, 3, 5).reshape(Do, Ho, Wo, C, -1)
    n = win.shape[-1]
    arg = (n - 1 - np.argmax(win[..., ::-1], axis=-1)) if last else np.argmax(win, axis=-1)
    g = np.zeros(win.shape, dtype=dout.dtype)
    np.put_along_axis(g, arg[..., None], dout[..., None], axis=-1)
    return g.reshape(Do, Ho, Wo, C, f[0], f[1], f[2]).transpose(0, 4, 1, 5, 2, 6, 3).reshape(D, H, W, C)


def interp_matrix(n_in, f, offset, n_out, clamp=True):
    """(n_out, n_in) weights of the linear interpolation by factor f (align_corners=False) followed by the crop at `offset`.
    clamp=False (fault injection): the upper neighbour past the far edge is dropped instead of clamped onto the last voxel."""
    dst = np.arange(n_out) + offset
    src = np.maximum((dst + 0.5) / f - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    w1 = np.clip(src - i0, 0.0, 1.0)
    A = np.zeros((n_out, n_in))
    A[np.arange(n_out), i0] += 1.0 - w1
    i1 = i0 + 1
    ok = i1 <= n_in - 1
    if clamp:
        i1 = np.minimum(i1, n_in - 1)
        ok = np.ones_like(ok)
    A[np.arange(n_out)[ok], i1[ok]] += w1[ok]
    return A


def upsample_backward(dout, in_shape, f, offset, fn=None, clamp=True, unit_weights=False):
    """Transposed trilinear interpolation + crop: din (in_shape) in float64.  fn: applied to dout first (np.abs: the scale T of
    the bound); unit_weights: every non-zero weight replaced by 1 (the scale of an error of the weights themselves)."""
    a = np.asarray(dout, dtype=np.float64)
    if fn is not None:
        a = fn(a)
    for d in range(3):
        A = interp_matrix(in_shape[d], f[d], offset[d], a.shape[d], clamp)
        if unit_weights:
            A = (A != 0).astype(np.float64)
        a = np.moveaxis(np.tensordot(A.T, a, axes=(1, d)), 0, d)
    return a


def upsample_fan_in(f):
    """The largest number of outputs that feed one input: along an axis of factor f > 1 input j is the lower neighbour of f
    outputs and the upper one of f more; factor 1 copies."""
    return int(np.prod([2 * v if v > 1 else 1 for v in f]))


def upsample_weight_error(in_shape, f):
    return sum(3 * U * (n + 1) for n, v in zip(in_shape, f) if v & (v - 1))


# ---- loss, head, Adam -------------------------------------------------------------------------------------------------------
def weighted_mse(p, t, w, count_all=None):
    """(loss, dL/dp, N, masked) in float64 from float32 arrays.  masked: some weighted error is non-zero, the mean runs over
    w > 0; else over all elements.  count_all (fault injection): force N = numel while keeping the mask."""
    p, t, w = (np.asarray(a, dtype=np.float64) for a in (p, t, w))
    d = p - t
    sc = w * d * d
    masked = bool(np.any(sc != 0))
    sel = w > 0
    n = int(sel.sum()) if masked else sc.size
    if count_all:
        n = sc.size
    loss = (sc[sel].sum() if masked else sc.sum()) / n
    dp = 2.0 * w * d / n
    if masked:
        dp = np.where(sel, dp, 0.0)
    return float(loss), dp, n, masked


def head_backward(z, p, dp, wc, wr):
    """z (M, cin), p / dp (M, cout), wc / wr (cout, cin): dz (M, cin), T = sum of |terms| of dz, dW (cout, cin) with its S,
    db (cout,) with its S; float64."""
    z, p, dp, wc, wr = (np.asarray(a, dtype=np.float64) for a in (z, p, dp, wc, wr))
    dl = dp * p * (1.0 - p)
    w = wc + wr
    dz = dl @ w
    T = np.abs(dl) @ np.abs(w)
    dW = dl.T @ z
    SW = np.sqrt((dl * dl).T @ (z * z))
    return dz, T, dW, SW, dl.sum(axis=0), np.sqrt((dl * dl).sum(axis=0)), dl


def adam_scalars(lr, b1, b2, eps, t):
    """The host-side f32 scalars of bsmi_unet_train_adam_step, as float64 values"""
    f = np.float32
    bc1 = f(1) - np.power(f(b1), f(t), dtype=np.float32)
    bc2 = f(1) - np.power(f(b2), f(t), dtype=np.float32)
    return dict(lr=float(f(lr)), b1=float(f(b1)), b2=float(f(b2)), eps=float(f(eps)), bc1=float(bc1), bc2_sqrt=float(np.sqrt(bc2, dtype=np.float32)))


def adam_moments(g, m, v, sc, grad_scale):
    g = np.asarray(g, np.float64) * float(np.float32(grad_scale))
    m1 = sc["b1"] * np.asarray(m, np.float64) + (1.0 - sc["b1"]) * g
    v1 = sc["b2"] * np.asarray(v, np.float64) + (1.0 - sc["b2"]) * g * g
    return m1, v1


def adam_update(m1, v1, sc, bias_correction=True):
    """the step -(lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps) in float64; bias_correction=False: the fault"""
    bc1, bc2s = (sc["bc1"], sc["bc2_sqrt"]) if bias_correction else (1.0, 1.0)
    return -(sc["lr"] / bc1) * (np.asarray(m1, np.float64) / (np.sqrt(np.asarray(v1, np.float64)) / bc2s + sc["eps"]))


# ---- weight and bias gradients -------------------------------------------------------------------------------------------------
def _taps(kernel):
    return [(dz, dy, dx) for dz in range(kernel[0]) for dy in range(kernel[1]) for dx in range(kernel[2])]


def weight_gradient(g, x, kernel):
    """g (Do, Ho, Wo, N) the interior of the masked gradient, x (Do + kz - 1, .., C) the slot's input region: dW (N, C, ntap) and
    S (N, C, ntap) = sqrt(sum g^2 x^2), float64."""
    g = np.asarray(g, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    Do, Ho, Wo, N = g.shape
    G = g.reshape(-1, N)
    G2 = G * G
    taps = _taps(kernel)
    dW = np.empty((N, x.shape[3], len(taps)))
    S = np.empty_like(dW)
    for t, (dz, dy, dx) in enumerate(taps):
        X = x[dz:dz + Do, dy:dy + Ho, dx:dx + Wo].reshape(-1, x.shape[3])
        dW[:, :, t] = G.T @ X
        S[:, :, t] = np.sqrt(G2.T @ (X * X))
    return dW, S


def bias_gradient(g):
    G = np.asarray(g, dtype=np.float64).reshape(-1, g.shape[-1])
    return G.sum(axis=0), np.sqrt((G * G).sum(axis=0))


def _edge_set(n, tile):
    """channels a sample must hold: first, last real, the first of the last (padded) tile, both sides of the first tile edge"""
    s = {0, n - 1, (n - 1) // tile * tile}
    if n > tile:
        s |= {tile - 1, tile}
    return s


def live_channels(a):
    """channels of a (.., C) tensor that hold a non-zero value (after a ReLU whole channels can be dead: their sums are exact
    zeros and say nothing about an accumulation)"""
    return np.flatnonzero(np.asarray(a).reshape(-1, a.shape[-1]).any(axis=0))


def wgrad_sample(N, C, ntap, tile_n, tile_c, rng, budget=WGRAD_SAMPLE, live_n=None, live_c=None):
    """(n indices, c indices): every tap of every (n, c) pair is taken; the sets hold the edge channels of _edge_set and seeded
    random ones -- live channels (live_n, live_c: live_channels of g and x) before dead ones --, about `budget` output elements
    in all (fewer where the slot is smaller)."""
    def pick(n, tile, per, live):
        s = sorted(_edge_set(n, tile))
        rest = [v for v in rng.permutation(n) if v not in s]
        if live is not None:      # the random ones among the live channels first
            alive = set(int(v) for v in live)
            rest = [v for v in rest if v in alive] + [v for v in rest if v not in alive]
        return np.array(sorted(s + [int(v) for v in rest[:max(0, per - len(s))]]), dtype=np.int64)
    c_idx = pick(C, tile_c, 6, live_c)                       # (a column of x costs a pass over every voxel per tap; a row of g is one more
    return pick(N, tile_n, max(6, budget // (ntap * len(c_idx))), live_n), c_idx   # column of the same product)


def _range_orders(nr, rng):
    return [np.arange(nr), np.arange(nr)[::-1], rng.permutation(nr), rng.permutation(nr)]


def _range_sums(P, split, lpr):
    """P (lines, Wo, columns) float64 products of one (c, tap): the f32 sum of every line range as the matrix pipe forms it.  One
    MFMA instruction contracts 2 voxels of a line (f32 families) or a chunk of 4 groups of 8 voxels, the last group of a line
    zero-filled, chunks running on over the lines of a range (split form): its products are added in float64 and rounded,
    instruction after instruction in f32.  -> (ranges, columns) float32"""
    nl, Wo, nn = P.shape
    grp = 8 if split else 2
    gpl = -(-Wo // grp)
    Pl = np.zeros((nl, gpl * grp, nn))
    Pl[:, :Wo] = P
    Q = Pl.reshape(nl, gpl, grp, nn).sum(axis=2)
    sums = []
    for r in range(-(-nl // lpr)):
        q = Q[r * lpr:(r + 1) * lpr].reshape(-1, nn)
        if split:
            pad = (-len(q)) % 4
            q = np.concatenate([q, np.zeros((pad, nn))]).reshape(-1, 4, nn).sum(axis=1)
        sums.append(np.cumsum(q.astype(np.float32), axis=0, dtype=np.float32)[-1])
    return np.array(sums, dtype=np.float32)


def wgrad_allowances(g, x, kernel, info, rng, n_idx=None, c_idx=None, n_seq=8):
    """(e_fmt, e_acc32) of one weight-gradient launch from the reference alone, on the sample (n_idx x c_idx x every tap).
    The ordered f32 sum (_range_sums, then the range sums in four orders: ascending, descending, two seeded shuffles -- float
    atomics order them by chance -- the largest error taken) runs on every sampled output channel where the launch has at most
    32 768 voxels, else on n_seq of them (the last real one among them): 6 x taps x that many ordered sums per launch.
    info: family ("wave-f32" / "tiled-f32" / "split-bf16"), tile, ranges, lines_per_range of the launch."""
    Do, Ho, Wo, N = g.shape
    C = x.shape[3]
    taps = _taps(kernel)
    if n_idx is None:
        n_idx, c_idx = wgrad_sample(N, C, len(taps), info["tile"][0], info["tile"][1], rng, live_n=live_channels(g), live_c=live_channels(x))
    split = info["family"] == "split-bf16"
    g32 = np.ascontiguousarray(np.asarray(g, dtype=np.float32)[..., n_idx]).reshape(-1, len(n_idx))
    G = g32.astype(np.float64)
    G2 = G * G
    if split:
        Gh, Gl = L.split_bf16(g32)
        Ghl = Gh + Gl
    if Do * Ho * Wo <= 32768:
        n_seq = len(n_idx)
    seq_cols = np.unique(np.concatenate([np.arange(min(n_seq - 1, len(n_idx))), [int(np.argmax(n_idx == N - 1))]]))
    nl = Do * Ho
    Gs = G[:, seq_cols].reshape(nl, Wo, -1)
    lpr = max(1, int(info["lines_per_range"]))
    nr = -(-nl // lpr)
    x32 = np.asarray(x, dtype=np.float32)
    tG32 = torch.from_numpy(g32)
    e_fmt = e_seq = e_blas = 0.0
    for c in c_idx:
        for (dz, dy, dx) in taps:
            xv32 = np.ascontiguousarray(x32[dz:dz + Do, dy:dy + Ho, dx:dx + Wo, c]).reshape(-1)
            xv = xv32.astype(np.float64)
            ref = xv @ G
            S = np.sqrt((xv * xv) @ G2)
            if split:
                xh, xl = L.split_bf16(xv32)
                e_fmt = max(e_fmt, L.norm_err(xh @ Ghl + xl @ Gh, ref, S))
            e_blas = max(e_blas, L.norm_err((torch.from_numpy(xv32) @ tG32).numpy().astype(np.float64), ref, S))
            sums = _range_sums(Gs * xv.reshape(nl, Wo, 1), split, lpr)
            for order in _range_orders(nr, rng):
                tot = np.cumsum(sums[order], axis=0, dtype=np.float32)[-1].astype(np.float64)
                e_seq = max(e_seq, L.norm_err(tot, ref[seq_cols], S[seq_cols]))
    return e_fmt, max(e_seq, e_blas)


def emulate_wgrad_f32_accumulation(g, x, kernel, info, order="ascending", seed=0):
    """dW (N, C, ntap) float32 as a launch of `info` ACCUMULATES it: the form's products (exact f32, or hi hi + lo hi + hi lo)
    summed in f32 per line range instruction by instruction (_range_sums), then the range sums added in f32 in `order`
    (ascending / descending / shuffled).  What tests/test_backward_cpu.py puts in the kernel's place."""
    g32, x32 = np.asarray(g, dtype=np.float32), np.asarray(x, dtype=np.float32)
    Do, Ho, Wo, N = g32.shape
    nl, split, lpr = Do * Ho, info["family"] == "split-bf16", max(1, int(info["lines_per_range"]))
    nr = -(-nl // lpr)
    order = {"ascending": np.arange(nr), "descending": np.arange(nr)[::-1], "shuffled": np.random.default_rng(seed).permutation(nr)}[order]
    G = g32.astype(np.float64).reshape(nl, Wo, N)
    if split:
        Gh, Gl = (a.reshape(nl, Wo, N) for a in L.split_bf16(g32))
    taps = _taps(kernel)
    out = np.zeros((N, x32.shape[3], len(taps)), dtype=np.float32)
    for c in range(x32.shape[3]):
        for t, (dz, dy, dx) in enumerate(taps):
            xv32 = x32[dz:dz + Do, dy:dy + Ho, dx:dx + Wo, c].reshape(nl, Wo, 1)
            if split:
                xh, xl = L.split_bf16(xv32)
                P = (Gh + Gl) * xh + Gh * xl
            else:
                P = G * xv32.astype(np.float64)
            out[:, c, t] = np.cumsum(_range_sums(P, split, lpr)[order], axis=0, dtype=np.float32)[-1]
    return out


def emulate_wgrad(g, x, kernel, info, drop_last_group=False, drop_last_range=False):
    """dW (N, C, ntap) as a launch of `info` forms it, float64 sums of the form's products (test_backward_cpu.py).
    drop_last_group: the last group of 8 voxels of every line never multiplied when Wo % 8 != 0; drop_last_range: the last line
    range of the launch never added."""
    g32, x32 = np.asarray(g, dtype=np.float32), np.asarray(x, dtype=np.float32)
    Do, Ho, Wo, N = g32.shape
    if drop_last_group and Wo % 8:
        g32 = g32.copy()
        g32[:, :, Wo // 8 * 8:] = 0
    if drop_last_range:
        lpr = int(info["lines_per_range"])
        keep = (-(-(Do * Ho) // lpr) - 1) * lpr
        g32 = g32.reshape(Do * Ho, Wo, N).copy()
        g32[keep:] = 0
        g32 = g32.reshape(Do, Ho, Wo, N)
    if info["family"] != "split-bf16":
        return weight_gradient(g32, x32, kernel)[0]
    gh, gl = L.split_bf16(g32)
    xh, xl = L.split_bf16(x32)
    return weight_gradient(gh + gl, xh, kernel)[0] + weight_gradient(gh, xl, kernel)[0]


def check_wgrad(got, g, x, kernel, info, rng, n_idx=None, c_idx=None, full=True):
    """One weight-gradient launch: got (N, C, ntap) (full) or the sampled block got[n_idx][:, c_idx] against float64, gate from the
    reference alone.  -> (ok, worst, g_acc, e_fmt, e_acc32)"""
    e_fmt, e_acc = wgrad_allowances(g, x, kernel, info, rng, None if full else n_idx, None if full else c_idx)
    g_acc = L.gate(e_fmt, e_acc)
    if full:
        ref, S = weight_gradient(g, x, kernel)
    else:
        ref, S = weight_gradient(np.asarray(g)[..., n_idx], np.asarray(x)[..., c_idx], kernel)
    sh = (ref.shape[0], -1)
    ok, worst = L.compare(np.asarray(got, dtype=np.float64).reshape(sh), ref.reshape(sh), S.reshape(sh), g_acc, U)
    return ok, worst, g_acc, e_fmt, e_acc


def reduction_allowance(terms32, ref, S, rng, group=256, trials=8):
    """The largest S-normalised error of f32 sums of the columns of terms32 (M, n) in the orders a reduction with float atomics
    can take: voxel order, its reverse, torch's CPU sum, and `trials` times the kernels' shape -- a seeded permutation of the terms
    cut into groups of `group` (what one thread or workgroup sums in sequence), the group sums added in sequence in that chance
    order -- plus the same shape over interleaved terms (thread t takes t, t + stride, ..).  Every column gives a sample of every
    order, so a tensor of three channels still yields some thirty."""
    t = np.ascontiguousarray(terms32, dtype=np.float32)
    M = len(t)

    def grouped(a):
        pad = (-len(a)) % group
        a = np.concatenate([a, np.zeros((pad, a.shape[1]), np.float32)]).reshape(-1, group, a.shape[1])
        part = np.cumsum(a, axis=1, dtype=np.float32)[:, -1]
        return np.cumsum(part, axis=0, dtype=np.float32)[-1].astype(np.float64)

    cands = [np.cumsum(t, axis=0, dtype=np.float32)[-1].astype(np.float64), np.cumsum(t[::-1], axis=0, dtype=np.float32)[-1].astype(np.float64),
             torch.from_numpy(t).sum(dim=0).numpy().astype(np.float64), grouped(t)]
    stride = max(1, -(-M // group))
    cands.append(grouped(np.concatenate([t[k::stride] for k in range(stride)])))
    for _ in range(trials):
        cands.append(grouped(t[rng.permutation(M)]))
    return max(L.norm_err(c, ref, S) for c in cands)


def check_bias(got, g, rng):
    """bias gradient (column sums of the interior of the masked gradient): exact f32 terms, so e_fmt = 0; e_acc32 from
    reduction_allowance: relu_bwd_pad_kernel sums per thread, then LDS atomics, then one global atomic per workgroup in an order
    that chance decides (colsum_kernel: per lane group, then atomics or the ordered fold)."""
    ref, S = bias_gradient(g)
    G32 = np.asarray(g, dtype=np.float32).reshape(-1, g.shape[-1])
    g_acc = L.gate(0.0, reduction_allowance(G32, ref, S, rng))
    ok, worst = L.compare(np.asarray(got, np.float64)[None], ref[None], S[None], g_acc, U)
    return ok, worst, g_acc


# ---- input gradient ---------------------------------------------------------------------------------------------------------
def dgrad_stage(gp, P, kernel, w, res=None, mirror=True, res_origin=None):
    """The input-gradient launch of a conv stage as a layer_ref.Stage over the padded masked gradient gp (border P, as the device
    holds it).  w (N, Cin, kz, ky, kx) the stage's weight.  res = (gp_last, P_last, crop, wr) for a pass's first stage with a
    residual branch: the columns of wr (N, Cin, 1, 1, 1) read the last stage's padded gradient crop / 2 before the voxel.
    mirror=False / res_origin (fault injection): taps not mirrored / the residual read at another origin.
    Output voxel v of the (Do + kz - 1, ..) input-gradient tensor reads gp at v + tap + P - (k - 1)."""
    w = np.asarray(w, dtype=np.float32)
    wt = w.transpose(1, 0, 2, 3, 4)
    if mirror:
        wt = wt[:, :, ::-1, ::-1, ::-1]
    org = tuple(P[d] - (kernel[d] - 1) for d in range(3))
    src = [(L.Dense(gp), org, gp.shape[3])]
    zeros = np.zeros(w.shape[1], dtype=np.float32)
    if res is None:
        return L.Stage(src, kernel, np.ascontiguousarray(wt), zeros, relu=False)
    gl, Pl, crop_, wr = res
    ro = tuple(Pl[d] - crop_[d] // 2 for d in range(3)) if res_origin is None else res_origin
    wrt = np.ascontiguousarray(np.asarray(wr, dtype=np.float32).transpose(1, 0, 2, 3, 4))
    return L.Stage(src, kernel, np.ascontiguousarray(wt), zeros, [(L.Dense(gl), ro, gl.shape[3])], wrt, zeros, relu=False)


def input_gradient(g, w, kernel, g_last=None, wr=None, crop_=None):
    """The same operation written directly (float64, whole tensor): g (Do, Ho, Wo, N) unpadded, w (N, Cin, kz, ky, kx); g_last the
    unpadded masked gradient of the pass's last stage, added through wr at offset crop / 2."""
    g = np.asarray(g, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    Do, Ho, Wo, _ = g.shape
    out = np.zeros((Do + kernel[0] - 1, Ho + kernel[1] - 1, Wo + kernel[2] - 1, w.shape[1]))
    for dz, dy, dx in _taps(kernel):
        out[dz:dz + Do, dy:dy + Ho, dx:dx + Wo] += g @ w[:, :, dz, dy, dx]
    if g_last is not None:
        o = tuple(c // 2 for c in crop_)
        gl = np.asarray(g_last, dtype=np.float64)
        out[o[0]:o[0] + gl.shape[0], o[1]:o[1] + gl.shape[1], o[2]:o[2] + gl.shape[2]] += gl @ np.asarray(wr, np.float64)[:, :, 0, 0, 0]
    return out


def dgrad_sample(shape, rng, n=2048):
    """rows of an input-gradient tensor on which its allowances are computed: the 8 corners (border rows that a single tap
    reaches), the last flat index and seeded random ones, at most n + 9"""
    D, H, W = shape[:3]
    M = D * H * W
    if M <= n:
        idx = np.arange(M)
    else:
        corners = [z * H * W + y * W + x for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)] + [M - 1]
        idx = np.unique(np.concatenate([corners, rng.integers(0, M, size=n)]))
    return idx // (H * W), (idx // W) % H, idx % W


def check_dgrad(got, stage, prec, split_k, g_out, rng, chunk_elems=4e7):
    """One input-gradient launch: got (D, H, W, Cin) against float64 of `stage` (dgrad_stage over the device's padded gradients),
    every element; the gate on dgrad_sample.  -> (ok, worst, vox of the failing chunk, g_acc, e_fmt, e_acc32, largest err / S)"""
    shape = got.shape
    gv = dgrad_sample(shape, rng)
    Xg = stage.rows(*gv)
    pre, S = stage.ref(Xg)
    e_fmt, e_acc = L.allowances(stage, Xg, pre, S, prec, False, split_k)
    g_acc = L.gate(e_fmt, e_acc)
    vox = L.all_voxels(shape)
    n, K = len(vox[0]), stage.W.shape[0]
    rows = max(256, int(chunk_elems // max(K, 1)))
    worst_es = 0.0
    for a in range(0, n, rows):
        cv = tuple(v[a:a + rows] for v in vox)
        pre, S = stage.ref(stage.rows(*cv))
        ok, worst = L.compare(got[cv].astype(np.float64), pre, S, g_acc, g_out)
        worst_es = max(worst_es, worst["max_err_over_S"])
        if not ok:
            return False, worst, cv, g_acc, e_fmt, e_acc, worst_es
    return True, worst, cv, g_acc, e_fmt, e_acc, worst_es


# ---- a whole step in float64 (tests/test_backward_cpu.py) -------------------------------------------------------------------------
def w5(a):
    a = np.asarray(a)
    return a[:, :, None] if a.ndim == 4 else a


def forward_chain(ops, sd, x):
    """Activations of every step of layer_ref.walk in float64 (heads: the sigmoid outputs (M, cout)); x (D, H, W, Cin).  The
    parameters are float32 values (layer_ref.Stage holds them as such)."""
    acts = [None] * len(ops)
    for i, o in enumerate(ops):
        if o["type"] == "input":
            acts[i] = np.asarray(x, dtype=np.float64)
        elif o["type"] == "conv":
            key = f"{o['prefix']}.conv_pass.{2 * o['conv']}"
            src = [(L.Dense(acts[s]), org, c) for s, org, c in o["src"]]
            res = [(L.Dense(acts[s]), org, c) for s, org, c in o["res"]] if o["res"] else None
            st = L.Stage(src, o["kernel"], w5(sd[key + ".weight"]), sd[key + ".bias"], res,
                         w5(sd[o["prefix"] + ".residual.0.weight"]) if res else None, sd[o["prefix"] + ".residual.0.bias"] if res else None)
            pre = st.rows(*L.all_voxels(o["shape"])) @ st.W + st.b
            acts[i] = np.maximum(pre, 0.0).reshape(o["shape"])
        elif o["type"] == "pool":
            acts[i] = L.maxpool(acts[o["src"]], o["factor"])
        elif o["type"] == "up":
            acts[i] = L.Upsampled(L.Dense(acts[o["src"]]), o["factor"], o["offset"], o["shape"]).full()
        else:
            z = acts[o["src"]].reshape(-1, acts[o["src"]].shape[3])
            wc, wr = (np.asarray(sd[f"{o['prefix']}.{k}.0.weight"], np.float64).reshape(o["shape"][3], -1) for k in ("conv_pass", "residual"))
            b = np.asarray(sd[o["prefix"] + ".conv_pass.0.bias"], np.float64) + np.asarray(sd[o["prefix"] + ".residual.0.bias"], np.float64)
            acts[i] = 1.0 / (1.0 + np.exp(-(z @ (wc + wr).T + b)))
    return acts


def _slot_ranges(src):
    out, b = [], 0
    for _, _, c in src:
        out.append((b, c))
        b += c
    return out


def backward_chain(ops, sd, acts, targets, weights):
    """The whole backward pass as the chain of this module's operations, float64: (loss, {parameter: gradient}, [dL/d(output of
    step)]).  targets / weights: per head (M, cout) arrays."""
    n = len(ops)
    dout = [None] * n
    grads, loss = {}, 0.0

    def add(i, a):
        dout[i] = a if dout[i] is None else dout[i] + a

    heads = [i for i, o in enumerate(ops) if o["type"] == "head"]
    gps = {}
    for i in range(n - 1, -1, -1):
        o = ops[i]
        if o["type"] == "head":
            h = heads.index(i)
            l, dp, _, _ = weighted_mse(acts[i], targets[h], weights[h])
            loss += l
            z = acts[o["src"]]
            wc, wr = (np.asarray(sd[f"{o['prefix']}.{k}.0.weight"], np.float64).reshape(o["shape"][3], -1) for k in ("conv_pass", "residual"))
            dz, _, dW, _, db, _, _ = head_backward(z.reshape(-1, z.shape[3]), acts[i], dp, wc, wr)
            add(o["src"], dz.reshape(z.shape))
            for k in ("conv_pass", "residual"):
                grads[f"{o['prefix']}.{k}.0.weight"] = dW.reshape(np.asarray(sd[f"{o['prefix']}.{k}.0.weight"]).shape)
                grads[f"{o['prefix']}.{k}.0.bias"] = db
        elif o["type"] == "up":
            add(o["src"], upsample_backward(dout[i], acts[o["src"]].shape, o["factor"], o["offset"]))
        elif o["type"] == "pool":
            add(o["src"], maxpool_backward(acts[o["src"]], dout[i], o["factor"]))
        elif o["type"] == "conv":
            ks, first = pass_kernels(ops, i)
            ci, last = o["conv"], o["conv"] == len(ks) - 1
            P = border_of(ks, ci)
            gp = masked_gradient(dout[i], acts[i], P)
            gps[i] = (gp, P)
            g = interior(gp, P)
            key = f"{o['prefix']}.conv_pass.{2 * ci}"
            w = w5(np.asarray(sd[key + ".weight"], np.float64))
            ext = tuple(o["shape"][d] + o["kernel"][d] - 1 for d in range(3))
            dW = np.zeros(w.shape)
            for (b, c), (s, org, _) in zip(_slot_ranges(o["src"]), o["src"]):
                dW[:, b:b + c] = weight_gradient(g, crop(acts[s], org, ext), o["kernel"])[0].reshape(w.shape[0], c, *o["kernel"])
            grads[key + ".weight"] = dW.reshape(np.asarray(sd[key + ".weight"]).shape)
            grads[key + ".bias"] = bias_gradient(g)[0]
            if last:
                wr = np.asarray(sd[o["prefix"] + ".residual.0.weight"], np.float64)
                dWr = np.zeros(wr.reshape(wr.shape[0], -1).shape)
                for (b, c), (s, org, _) in zip(_slot_ranges(o["res"]), o["res"]):
                    dWr[:, b:b + c] = weight_gradient(g, crop(acts[s], org, o["shape"][:3]), (1, 1, 1))[0][:, :, 0]
                grads[o["prefix"] + ".residual.0.weight"] = dWr.reshape(wr.shape)
                grads[o["prefix"] + ".residual.0.bias"] = bias_gradient(g)[0]
            if ci > 0:
                add(o["src"][0][0], input_gradient(g, w, o["kernel"]))
            elif ops[o["src"][0][0]]["type"] != "input":
                gl, Pl = gps[first + len(ks) - 1]
                wr = w5(np.asarray(sd[o["prefix"] + ".residual.0.weight"], np.float64))
                dcat = input_gradient(g, w, o["kernel"], interior(gl, Pl), wr, pass_crop(ks))
                parts = scatter(dcat, [(org, c) for _, org, c in o["src"]], [acts[s].shape for s, _, _ in o["src"]])
                for (s, _, _), a in zip(o["src"], parts):
                    add(s, a)
    return loss, grads, dout


# ---- the checks both suites apply (got: what the device, or an emulation in its place, holds) ---------------------------------------
def check_masked(got_gp, dout, y, P):
    """the padded masked gradient, border included: bit-equal"""
    return bool(np.array_equal(got_gp, masked_gradient(dout, y, P))) and border_nonzero(got_gp, P) == 0


def check_split(hi, lo, gp):
    """the split copy: hi = bf16(v), lo = bf16(v - hi) of every value of the padded masked gradient, bit-equal"""
    rh, rl = L.split_bf16(gp)
    return bool(np.array_equal(hi.astype(np.float64), rh) and np.array_equal(lo.astype(np.float64), rl))


def check_upsample_backward(got, dout, in_shape, f, offset):
    """|got - ref| <= (n + 3) 2^-24 T(|dout|) (+ the weights' own rounding for a factor that is no power of two): every product
    g * wt carries the roundings of the three-factor weight and of the product (3), the sum of at most n of them n more.
    -> (ok, number of elements off, largest error / bound)"""
    ref = upsample_backward(dout, in_shape, f, offset)
    T = upsample_backward(dout, in_shape, f, offset, np.abs)
    bound = (upsample_fan_in(f) + 3) * U * T
    we = upsample_weight_error(in_shape, f)
    if we:
        bound = bound + we * upsample_backward(dout, in_shape, f, offset, np.abs, unit_weights=True)
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = err > bound
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return not bad.any(), int(bad.sum()), float(ratio.max())


def check_loss_gradient(got_dp, p, t, w):
    """dL/dp: the mask (zero exactly where the reference is zero) bit-equal, the values to 4 * 2^-24 relative element-wise:
    f32 roundings of p - t, of w (p - t), of 1 / N and of the last product (2 * is exact)."""
    _, dp, n, masked = weighted_mse(p, t, w)
    got = np.asarray(got_dp, np.float64)
    mask_ok = bool(np.array_equal(got != 0, dp != 0))
    return mask_ok and bool(np.all(np.abs(got - dp) <= 4 * U * np.abs(dp))), n, masked


def check_adam(p0, g, m0, v0, p1, m1, v1, sc, grad_scale):
    """One Adam step element-wise from the values before the step: m and v to 4 * 2^-24 relative; the update, from the moments
    as stored after the step, to 8 * 2^-24 |delta| + 2^-24 |p|."""
    rm, rv = adam_moments(g, m0, v0, sc, grad_scale)
    m1, v1, p0, p1 = (np.asarray(a, np.float64) for a in (m1, v1, p0, p1))
    ok_m = bool(np.all(np.abs(m1 - rm) <= 4 * U * np.abs(rm)))
    ok_v = bool(np.all(np.abs(v1 - rv) <= 4 * U * np.abs(rv)))
    delta = adam_update(m1, v1, sc)
    ok_p = bool(np.all(np.abs((p1 - p0) - delta) <= 8 * U * np.abs(delta) + U * np.abs(p0)))
    return ok_m, ok_v, ok_p


# ---- the cases both suites run ----------------------------------------------------------------------------------------------
C_NET = {"in_channels": 1, "num_fmaps": 12, "fmap_inc_factor": 5, "downsample_factors": [[1, 2, 2], [1, 2, 2]],
         "kernel_size_down": [[[3, 3, 3], [3, 3, 3]]] * 3, "kernel_size_up": [[[3, 3, 3], [3, 3, 3]]] * 2, "outputs": {"3d_affs": {"dims": 6}}}
# Stage outputs (Do, Ho, Wo, C) at this input: (19,46,54,12) (17,44,52,12) | (15,20,24,60) (13,18,22,60) | (11,7,9,300) (9,5,7,300)
# | (7,8,12,60) (5,6,10,60) | (3,10,18,12) (1,8,16,12).  Every level above the bottom one has an even Wo by construction (it is pooled
# by 2 or is 2 n + crop), so Wo % 8 in {1, 7} exists only among the 300-channel stages (9 and 7); the 12- and 60-channel ones
# have Wo % 8 in {2, 6} (54, 18 / 22, 10): the last group of 8 of a line is partial at every width.  H != W; 9 * 5 = 45 lines of the
# second 300-channel stage are cut into ranges of 2 (23 ranges, the last with one line); 19 * 46 = 874 lines > 32 ranges.
C_SHAPE = (21, 48, 56)


def smallest_shape(nc, good):
    """the smallest input extent per axis that layer_ref.walk admits for the net, searched with the other axes at the admissible
    shape `good` (the axes are independent)"""
    out = []
    for d in range(3):
        for n in range(1, good[d] + 1):
            shp = list(good)
            shp[d] = n
            try:
                L.walk(nc, shp)
            except (ValueError, AssertionError):
                continue
            out.append(n)
            break
    L.walk(nc, out)
    return tuple(out)


def wgrad_tiles(family, N, C):
    """(tile_n, tile_c) a launch of `family` uses for a slot of N x C channels (launch_wgrad_x3_k / the f32 launcher)"""
    if family == "split-bf16":
        return (32 if N <= 32 else (64 if N <= 64 else 128), 32 if C <= 32 else 64)
    return (128, 128) if (N > 32 and C > 32) else (32, 64)


def wgrad_plan(arith, N, C, nlines, trows, det=False):
    """What the launcher runs for a slot, restated for the CPU self-test (the GPU suite reads it from the device's step info):
    dict(family, tile, ranges, lines_per_range)."""
    if arith == "split-bf16":
        tn, tc = wgrad_tiles("split-bf16", N, C)
        blocks = -(-N // tn) * -(-C // tc)
        zs = max(1, min(nlines, 4096 // max(1, blocks * trows)))
        if det:
            zs = min(zs, 32)
        fam = "split-bf16"
    else:
        tiled = N > 32 and C > 32
        tn, tc = wgrad_tiles("f32", N, C)
        blocks = (-(-N // 128) * -(-C // 128)) if tiled else (-(-N // 32) * -(-C // 64))
        zs = 1 if det else max(1, min(nlines, (2048 if tiled else 8192) // max(1, blocks * trows)))
        fam = "tiled-f32" if tiled else "wave-f32"
    lpr = -(-nlines // zs)
    return dict(family=fam, tile=(tn, tc), ranges=-(-nlines // lpr), lines_per_range=lpr)
