"""What the per-launch comparison of the backward pass (tests/bwd_ref.py, tests/test_backward_gpu.py) has to be able to tell.  No GPU.

  reference against autograd   chained over a small net, bwd_ref's operations reproduce torch's float64 autograd of the whole
                               training step to 1e-12 of each tensor's largest entry: the loss, every parameter gradient and
                               every activation gradient (nets: the golden affs_f4i2 at its smallest admissible input and the
                               two-slot 12 / 60 / 300 net at the ragged shape of case C -- the shapes of the GPU suite)
  correct emulations pass      the kernels' arithmetic put in the kernel's place passes the gate the MI355X is held to: the
                               split-bf16 products hi hi + lo hi + hi lo, and the launch's own f32 accumulation -- per line range
                               instruction by instruction, then the range sums ascending, descending and shuffled
  faulty emulations are refused, each at the shapes of case C: the last group of 8 voxels of a line dropped (Wo % 8 != 0), the
                               last line range of a cut launch dropped, a tap not mirrored in the input gradient, the residual
                               columns omitted or read at offset 0 instead of crop / 2, a second slot's cbase off by one tile,
                               the last real channel of the last row missing, the pool gradient at the LAST maximum, the upper
                               interpolation neighbour not clamped at the far edge, a non-zero border voxel, `lo` planes dropped
                               from the split copy, N of the loss over all elements, Adam without bias correction; and on a
                               synthetic 65 -> 65 weight-gradient stage (the tile edges of case E, tests/edge_nets.py): the second
                               C-tile's one real channel missing, row 64 zeroed, that channel leaking into column 63, one product
                               off by one bf16 ulp

Wall time: about 4 min on 8 threads (the float64 step of case C is computed once and shared).

Gates as in bwd_ref: from the reference alone.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bwd_ref as B
import layer_ref as L

torch.set_num_threads(min(16, os.cpu_count() or 1))
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the nets -----------------------------------------------------------------------------------------------------------------
def golden_net():
    from test_unet_gpu import _load, _net_config
    d, sd, meta = _load(GOLDEN_DIR, "affs_f4i2")
    nc = _net_config(meta)
    return nc, sd, B.smallest_shape(nc, d["raw_u8"].shape[-3:])


def c_net():
    from bootstrapper_amd.synth import synthetic_state_dict
    return B.C_NET, synthetic_state_dict(B.C_NET, 3), B.C_SHAPE


def step_data(nc, sd, shape, seed=0):
    """(ops, x, targets, weights): a random input block, binary targets and weights with a fifth of them zero"""
    rng = np.random.default_rng(seed)
    ops = L.walk(nc, shape)
    x = (rng.random(ops[0]["shape"], dtype=np.float32) * 2 - 1).astype(np.float32)
    ts, ws = [], []
    for o in ops:
        if o["type"] == "head":
            m = int(np.prod(o["shape"][:3]))
            ts.append((rng.random((m, o["shape"][3])) > 0.5).astype(np.float32))
            w = rng.random((m, o["shape"][3])).astype(np.float32)
            w[rng.random(w.shape) < 0.2] = 0
            ws.append(w)
    return ops, x, ts, ws


_CHAIN = {}


def chain(which):
    """the float64 step of a net, computed once and shared: (ops, sd, acts, loss, grads, dout)"""
    if which not in _CHAIN:
        nc, sd, shape = golden_net() if which == "golden" else c_net()
        ops, x, ts, ws = step_data(nc, sd, shape)
        acts = B.forward_chain(ops, sd, x)
        loss, grads, dout = B.backward_chain(ops, sd, acts, ts, ws)
        _CHAIN[which] = (ops, sd, x, ts, ws, acts, loss, grads, dout)
    return _CHAIN[which]


def autograd_step(ops, sd, x, ts, ws):
    """torch float64 autograd of the same step, built from the walk: (loss, parameter gradients, activation gradients)"""
    P = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)).requires_grad_(True) for k, v in sd.items()}
    w5 = lambda t: t[:, :, None] if t.dim() == 4 else t

    def cropped(t, org, ext):
        return t[:, :, org[0]:org[0] + ext[0], org[1]:org[1] + ext[1], org[2]:org[2] + ext[2]]

    acts, loss, h = [None] * len(ops), 0.0, 0
    for i, o in enumerate(ops):
        if o["type"] == "input":
            a = torch.from_numpy(np.ascontiguousarray(x.astype(np.float64).transpose(3, 0, 1, 2)))[None]
        elif o["type"] == "conv":
            ext = tuple(o["shape"][d] + o["kernel"][d] - 1 for d in range(3))
            key = f"{o['prefix']}.conv_pass.{2 * o['conv']}"
            a = F.conv3d(torch.cat([cropped(acts[s], org, ext) for s, org, _ in o["src"]], dim=1), w5(P[key + ".weight"]), P[key + ".bias"])
            if o["res"]:
                r = torch.cat([cropped(acts[s], org, o["shape"][:3]) for s, org, _ in o["res"]], dim=1)
                a = a + F.conv3d(r, w5(P[o["prefix"] + ".residual.0.weight"]), P[o["prefix"] + ".residual.0.bias"])
            a = torch.relu(a)
        elif o["type"] == "pool":
            a = F.max_pool3d(acts[o["src"]], tuple(o["factor"]), stride=tuple(o["factor"]))
        elif o["type"] == "up":
            up = F.interpolate(acts[o["src"]], scale_factor=tuple(float(f) for f in o["factor"]), mode="trilinear")
            a = cropped(up, o["offset"], o["shape"][:3])
        else:
            z = acts[o["src"]]
            y = F.conv3d(z, w5(P[o["prefix"] + ".conv_pass.0.weight"]), P[o["prefix"] + ".conv_pass.0.bias"]) + \
                F.conv3d(z, w5(P[o["prefix"] + ".residual.0.weight"]), P[o["prefix"] + ".residual.0.bias"])
            a = torch.sigmoid(y)
            p = a[0].permute(1, 2, 3, 0).reshape(-1, o["shape"][3])
            t, w = torch.from_numpy(ts[h].astype(np.float64)), torch.from_numpy(ws[h].astype(np.float64))
            sc = w * (p - t) ** 2
            loss = loss + (torch.mean(torch.masked_select(sc, w > 0)) if len(torch.nonzero(sc)) != 0 else torch.mean(sc))
            h += 1
        if o["type"] != "input" and o["type"] != "head":
            a.retain_grad()
        acts[i] = a
    loss.backward()
    kept = [o["type"] in ("conv", "pool", "up") for o in ops]
    return float(loss.detach()), {k: v.grad.numpy() for k, v in P.items()}, \
        [a.grad[0].permute(1, 2, 3, 0).numpy() if k else None for a, k in zip(acts, kept)]


@pytest.mark.parametrize("which", ["golden", "c"])
def test_reference_reproduces_float64_autograd(which):
    ops, sd, x, ts, ws, acts, loss, grads, dout = chain(which)
    a_loss, a_grads, a_dout = autograd_step(ops, sd, x, ts, ws)
    assert abs(loss - a_loss) <= 1e-12 * abs(a_loss)
    assert set(grads) == set(a_grads)
    worst = 0.0
    for k, ref in a_grads.items():
        e = np.abs(grads[k].reshape(ref.shape) - ref).max() / np.abs(ref).max()
        worst = max(worst, e)
        assert e <= 1e-12, (k, e)
    n_act = 0
    for i, ref in enumerate(a_dout):
        if ref is None:
            continue
        n_act += 1
        e = np.abs(dout[i] - ref).max() / np.abs(ref).max()
        worst = max(worst, e)
        assert e <= 1e-12, (i, ops[i]["type"], e)
    assert n_act == len([o for o in ops if o["type"] in ("conv", "pool", "up")])
    print(f"{which}: loss {loss:.9f}, {len(grads)} parameter and {n_act} activation gradients, largest relative difference {worst:.2e}")


def test_ties_at_zero_are_common_and_go_to_the_first_maximum():
    """after a ReLU whole pooling windows are zero: the rule that decides them is exercised by the case itself"""
    ops, sd, x, ts, ws, acts, *_ = chain("c")
    i = next(i for i, o in enumerate(ops) if o["type"] == "pool")
    a, f = acts[ops[i]["src"]], ops[i]["factor"]
    D, H, W, C = a.shape
    win = a.reshape(D // f[0], f[0], H // f[1], f[1], W // f[2], f[2], C).transpose(0, 2, 4, 6, 1, 3, 5).reshape(-1, f[0] * f[1] * f[2])
    ties = (win == win.max(axis=1, keepdims=True)).sum(axis=1) > 1
    assert ties.mean() > 0.01, ties.mean()


# ---- the device's tensors of case C, as float32 -----------------------------------------------------------------------------------
def c_tensors():
    ops, sd, x, ts, ws, acts, loss, grads, dout = chain("c")
    a32 = [None if a is None else a.astype(np.float32) for a in acts]
    d32 = [None if d is None else d.astype(np.float32) for d in dout]
    return ops, sd, a32, d32


def conv_step(ops, prefix, ci):
    return next(i for i, o in enumerate(ops) if o["type"] == "conv" and o["prefix"] == prefix and o["conv"] == ci)


def wgrad_operands(ops, a32, d32, i, slot=0, residual=False):
    """(g, x, kernel, cbase, N, C) of one weight-gradient launch of conv step i"""
    o = ops[i]
    ks, _ = B.pass_kernels(ops, i)
    P = B.border_of(ks, o["conv"])
    g = B.interior(B.masked_gradient(d32[i], a32[i], P), P)
    srcs = o["res"] if residual else o["src"]
    kernel = (1, 1, 1) if residual else o["kernel"]
    s, org, c = srcs[slot]
    ext = tuple(o["shape"][d] + kernel[d] - 1 for d in range(3))
    cbase = sum(cc for _, _, cc in srcs[:slot])
    return g, B.crop(a32[s], org, ext), kernel, cbase, o["shape"][3], c


WGRAD_LAUNCHES = [("unet.l_conv.0", 1, 0, False), ("unet.l_conv.1", 0, 0, False), ("unet.l_conv.1", 1, 0, False), ("unet.l_conv.2", 1, 0, False),
                  ("unet.r_conv.0.0", 0, 1, False), ("unet.r_conv.0.1", 1, 0, True)]


@pytest.mark.parametrize("arith", ["f32", "split-bf16", "f32+det", "split-bf16+det"])
@pytest.mark.parametrize("prefix,ci,slot,residual", WGRAD_LAUNCHES)
def test_weight_gradient_emulations(prefix, ci, slot, residual, arith):
    """The emulation of a launch's arithmetic passes; the same sums with the last group of 8 voxels of every line, the last line
    range, or the last real channel of the tile's last row left out are refused."""
    ops, sd, a32, d32 = c_tensors()
    i = conv_step(ops, prefix, ci)
    g, x, kernel, cbase, N, C = wgrad_operands(ops, a32, d32, i, slot, residual)
    Do, Ho, Wo, _ = g.shape
    info = B.wgrad_plan(arith.split("+")[0], N, C, Do * Ho, kernel[0] * kernel[1], det=arith.endswith("+det"))
    rng = np.random.default_rng(5)
    good = B.emulate_wgrad(g, x, kernel, info).astype(np.float32)
    ok, worst, g_acc, e_fmt, e_acc = B.check_wgrad(good, g, x, kernel, info, rng)
    print(f"{prefix} conv {ci} slot {slot} {arith}: {info}  Wo {Wo}  e_fmt {e_fmt:.2e} e_acc32 {e_acc:.2e} worst err/S {worst['max_err_over_S']:.2e}")
    assert ok, worst
    # ... and so does the launch's own accumulation: f32 per line range, instruction by instruction, then the range sums, in each
    # order (the 300 x 300 stage on the rows and columns of the gate's sample: 2.4 M sums otherwise)
    n_idx, c_idx = B.wgrad_sample(N, C, kernel[0] * kernel[1] * kernel[2], info["tile"][0], info["tile"][1], np.random.default_rng(5))
    for order in ("ascending", "descending", "shuffled"):
        acc = B.emulate_wgrad_f32_accumulation(g[..., n_idx], x[..., c_idx], kernel, info, order)
        ok, worst = B.check_wgrad(acc, g, x, kernel, info, np.random.default_rng(5), n_idx, c_idx, full=False)[:2]
        assert ok, (order, worst)
    if Wo % 8:
        bad = B.emulate_wgrad(g, x, kernel, info, drop_last_group=True).astype(np.float32)
        assert not B.check_wgrad(bad, g, x, kernel, info, np.random.default_rng(5))[0], "last group of 8 voxels of a line dropped"
    if info["ranges"] > 1:
        bad = B.emulate_wgrad(g, x, kernel, info, drop_last_range=True).astype(np.float32)
        assert not B.check_wgrad(bad, g, x, kernel, info, np.random.default_rng(5))[0], "last line range dropped"
    bad = good.copy()
    bad[N - 1, C - 1, :] = 0
    assert not B.check_wgrad(bad, g, x, kernel, info, np.random.default_rng(5))[0], "last real channel of the last row missing"


def test_partial_last_group_is_exercised_at_every_width():
    """among the launches above a stage of each width -- 12, 60, 300 output channels -- has lines whose last group of 8 is partial"""
    ops = L.walk(B.C_NET, B.C_SHAPE)
    widths = {ops[conv_step(ops, prefix, ci)]["shape"][3] for prefix, ci, _, _ in WGRAD_LAUNCHES if ops[conv_step(ops, prefix, ci)]["shape"][2] % 8}
    assert widths == {12, 60, 300}, widths


def test_second_slot_cbase_off_by_one_tile_is_refused():
    """r_conv.0.0 conv 0 reads the skip (12 channels, cbase 0) and the upsampled map (60 channels, cbase 12): the second slot's
    columns written one tile further are refused -- through the columns it leaves empty and those it overwrites."""
    ops, sd, a32, d32 = c_tensors()
    i = conv_step(ops, "unet.r_conv.0.0", 0)
    rng = np.random.default_rng(6)
    parts = [wgrad_operands(ops, a32, d32, i, sl) for sl in range(2)]
    N, ct = parts[0][4], sum(p[5] for p in parts)
    infos = [B.wgrad_plan("split-bf16", N, p[5], p[0].shape[0] * p[0].shape[1], 9) for p in parts]
    assert parts[1][3] == 12
    for shift in (0, infos[1]["tile"][1]):
        dW = np.zeros((N, ct + 64, 27), dtype=np.float32)
        for (g, x, kernel, cbase, _, C), info, sh in zip(parts, infos, (0, shift)):
            dW[:, cbase + sh:cbase + sh + C] += B.emulate_wgrad(g, x, kernel, info).astype(np.float32)
        dW = dW[:, :ct]
        oks = [B.check_wgrad(dW[:, p[3]:p[3] + p[5]], p[0], p[1], p[2], info, rng)[0] for p, info in zip(parts, infos)]
        assert all(oks) == (shift == 0), (shift, oks)


# ---- a weight-gradient stage on the tile edges (tests/edge_nets.py, tests/test_backward_edges_gpu.py) -------------------------------
_EDGE_WGRAD = {}


def edge_wgrad_stage():
    """65 -> 65 channels, 3x3x3, output (3, 10, 11): N = 65 is one row over the 64-row tile (the 128-row tile runs), C = 65 puts one
    real channel into a second 64-channel C-tile.  g: a masked gradient (half of it exact zeros), x: post-ReLU activations.  Made once."""
    if not _EDGE_WGRAD:
        rng = np.random.default_rng(65)
        g = (rng.standard_normal((3, 10, 11, 65)) * (rng.random((3, 10, 11, 65)) > 0.5)).astype(np.float32)
        x = np.maximum(rng.standard_normal((5, 12, 13, 65)), 0).astype(np.float32)
        _EDGE_WGRAD.update(g=g, x=x)
    return _EDGE_WGRAD["g"], _EDGE_WGRAD["x"]


@pytest.mark.parametrize("arith", ["f32", "split-bf16", "split-bf16+det"])
def test_weight_gradient_stage_with_65_channels(arith):
    """The emulations of the launch pass; refused are: the one real channel of the second C-tile never written, or written from the
    padding channel beside it (zeros); row 64 -- the first of the tile's second half of 64 -- zeroed; the last real column of the
    first C-tile (c = 63) with one product of every sum off by one bf16 ulp of its operand (f32 and split-bf16 both hold more
    than bf16's 8 bits); the second C-tile's channel also added into c = 63 (a padding column leaking into its neighbour)."""
    g, x = edge_wgrad_stage()
    kernel, N, C = (3, 3, 3), 65, 65
    Do, Ho, Wo, _ = g.shape
    info = B.wgrad_plan(arith.split("+")[0], N, C, Do * Ho, 9, det=arith.endswith("+det"))
    assert info["tile"] == ((128, 64) if arith.startswith("split") else (128, 128)), info
    check = lambda dw: B.check_wgrad(dw, g, x, kernel, info, np.random.default_rng(5))
    good = B.emulate_wgrad(g, x, kernel, info).astype(np.float32)
    ok, worst, g_acc, e_fmt, e_acc = check(good)
    print(f"65 x 65 {arith}: {info}  e_fmt {e_fmt:.2e} e_acc32 {e_acc:.2e} worst err/S {worst['max_err_over_S']:.2e}")
    assert ok, worst
    for order in ("ascending", "descending", "shuffled"):
        assert check(B.emulate_wgrad_f32_accumulation(g, x, kernel, info, order))[0], order
    bad = good.copy()
    bad[:, 64, :] = 0
    assert not check(bad)[0], "the second C-tile's real channel never written"
    bad = good.copy()
    bad[64, :, :] = 0
    assert not check(bad)[0], "row 64 zeroed"
    bad = good.copy()
    bad[:, 63, :] += good[:, 64, :]
    assert not check(bad)[0], "the second C-tile's channel added into the last column of the first"
    # one product per sum: the voxel with the largest |x| of channel 63 under the centre tap, its x off by one bf16 ulp
    xc = x[1:1 + Do, 1:1 + Ho, 1:1 + Wo, 63]
    v = np.unravel_index(int(np.argmax(np.abs(xc) * np.abs(g).max(axis=3))), xc.shape)
    ulp = 2.0 ** (np.floor(np.log2(abs(float(xc[v])))) - 7)
    bad = good.copy()
    bad[:, 63, 13] += (g[v].astype(np.float64) * ulp).astype(np.float32)
    ok, worst = check(bad)[:2]
    print(f"65 x 65 {arith}: one bf16 ulp of one product: err/S {worst['max_err_over_S']:.2e} against g_acc {g_acc:.2e}")
    assert not ok, "one product of column 63 off by one bf16 ulp"


# ---- input gradients ---------------------------------------------------------------------------------------------------------------
def dgrad_operands(ops, sd, a32, d32, prefix, ci):
    i = conv_step(ops, prefix, ci)
    ks, first = B.pass_kernels(ops, i)
    P = B.border_of(ks, ci)
    gp = B.masked_gradient(d32[i], a32[i], P)
    w = B.w5(sd[f"{prefix}.conv_pass.{2 * ci}.weight"])
    res = None
    if ci == 0:
        j = first + len(ks) - 1
        Pl = B.border_of(ks, len(ks) - 1)
        res = (B.masked_gradient(d32[j], a32[j], Pl), Pl, B.pass_crop(ks), B.w5(sd[prefix + ".residual.0.weight"]))
    return gp, P, ops[i]["kernel"], w, res


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("prefix,ci", [("unet.l_conv.1", 0), ("unet.l_conv.1", 1), ("unet.l_conv.2", 0), ("unet.r_conv.0.0", 0)])
def test_input_gradient_emulations(prefix, ci, prec):
    """The emulation of the launch's products passes its gate; taps that are not mirrored, residual columns that are left out or
    read at offset 0 instead of crop / 2 are refused."""
    ops, sd, a32, d32 = c_tensors()
    gp, P, kernel, w, res = dgrad_operands(ops, sd, a32, d32, prefix, ci)
    st = B.dgrad_stage(gp, P, kernel, w, res)
    shape = tuple(gp.shape[d] - 2 * P[d] + kernel[d] - 1 for d in range(3)) + (w.shape[1],)
    vox = L.all_voxels(shape)
    g_out = L.G_OUT[prec]

    def run(stage):
        got = L.store(stage.emulate(stage.rows(*vox), prec), prec).reshape(shape)
        return B.check_dgrad(got, st, prec, False, g_out, np.random.default_rng(7))

    ok, worst, _, g_acc, e_fmt, e_acc, es = run(st)
    print(f"{prefix} conv {ci} {prec}: K {st.W.shape[0]} e_fmt {e_fmt:.2e} e_acc32 {e_acc:.2e} largest err/S {es:.2e}")
    assert ok, worst
    # ... and agrees with the operation written directly
    direct = B.input_gradient(B.interior(gp, P), w, kernel, B.interior(res[0], res[1]) if res else None, res[3] if res else None, res[2] if res else None)
    assert np.abs(st.ref(st.rows(*vox))[0].reshape(shape) - direct).max() <= 1e-12 * np.abs(direct).max()
    assert not run(B.dgrad_stage(gp, P, kernel, w, res, mirror=False))[0], "taps not mirrored"
    if res:
        assert not run(B.dgrad_stage(gp, P, kernel, w, None))[0], "residual columns omitted"
        gl, Pl, crop_, wr = res
        pad = [(c, c) for c in crop_] + [(0, 0)]   # room for the displaced reads
        wide = (np.pad(gl, pad), tuple(Pl[d] + crop_[d] for d in range(3)), crop_, wr)
        moved = B.dgrad_stage(gp, P, kernel, w, wide, res_origin=tuple(wide[1]))
        assert not run(moved)[0], "residual read at offset 0"


# ---- routing, interpolation, borders, split copy ------------------------------------------------------------------------------------
def test_pool_gradient_at_the_last_maximum_is_refused():
    ops, sd, a32, d32 = c_tensors()
    for i, o in enumerate(ops):
        if o["type"] != "pool":
            continue
        x = a32[o["src"]]
        ref = B.maxpool_backward(x, d32[i], o["factor"])
        assert np.count_nonzero(ref) == np.count_nonzero(d32[i])      # every window's gradient lands on exactly one voxel
        assert not np.array_equal(B.maxpool_backward(x, d32[i], o["factor"], last=True), ref), i


def test_upsampling_backward_bound_and_unclamped_neighbour():
    """f32 emulation of the scatter form (every share rounded, summed in f32) passes; the upper neighbour dropped instead of
    clamped at the far edge is refused wherever the crop keeps the last output."""
    ops, sd, a32, d32 = c_tensors()
    seen_edge = False
    for i, o in enumerate(ops):
        if o["type"] != "up":
            continue
        in_shape = a32[o["src"]].shape
        got = B.upsample_backward(d32[i], in_shape, o["factor"], o["offset"]).astype(np.float32)
        ok, nbad, ratio = B.check_upsample_backward(got, d32[i], in_shape, o["factor"], o["offset"])
        assert ok, (i, nbad, ratio)
        bad = B.upsample_backward(d32[i], in_shape, o["factor"], o["offset"], clamp=False).astype(np.float32)
        reaches_edge = any(o["offset"][d] + o["shape"][d] == in_shape[d] * o["factor"][d] and o["factor"][d] > 1 for d in range(3))
        if reaches_edge:
            seen_edge = True
            assert not B.check_upsample_backward(bad, d32[i], in_shape, o["factor"], o["offset"])[0], i
    assert seen_edge, "no upsampling step of the case keeps its last output voxel: the fault could not show"


def test_border_split_copy_and_masking_faults_are_refused():
    ops, sd, a32, d32 = c_tensors()
    i = conv_step(ops, "unet.l_conv.1", 1)
    ks, _ = B.pass_kernels(ops, i)
    P = B.border_of(ks, 1)
    assert P == (2, 2, 2)
    gp = B.masked_gradient(d32[i], a32[i], P)
    assert B.check_masked(gp, d32[i], a32[i], P)
    bad = gp.copy()
    bad[0, 1, 1, 3] = np.float32(1e-30)
    assert not B.check_masked(bad, d32[i], a32[i], P) and B.border_nonzero(bad, P) == 1
    bad = gp.copy()
    y0 = np.argwhere(a32[i] <= 0)[0]
    bad[y0[0] + 2, y0[1] + 2, y0[2] + 2, y0[3]] = d32[i][tuple(y0)]          # a gradient let through where Y = 0
    assert d32[i][tuple(y0)] != 0 and not B.check_masked(bad, d32[i], a32[i], P)
    hi, lo = L.split_bf16(gp)
    assert B.check_split(hi.astype(np.float32), lo.astype(np.float32), gp)
    assert np.count_nonzero(lo) > 0 and not B.check_split(hi.astype(np.float32), np.zeros_like(gp), gp), "lo planes dropped"
    assert not B.check_split(L.bf16_rne(gp * np.float32(1 + 2.0 ** -7)), lo.astype(np.float32), gp)


# ---- loss and Adam -------------------------------------------------------------------------------------------------------------------
def test_loss_count_over_all_elements_is_refused():
    ops, sd, x, ts, ws, acts, *_ = chain("c")
    p, t, w = acts[-1].astype(np.float32), ts[0], ws[0]
    loss, dp, n, masked = B.weighted_mse(p, t, w)
    assert masked and n == int((w > 0).sum()) < w.size
    ok, n2, _ = B.check_loss_gradient(dp.astype(np.float32), p, t, w)
    assert ok and n2 == n
    bad = B.weighted_mse(p, t, w, count_all=True)[1].astype(np.float32)
    assert not B.check_loss_gradient(bad, p, t, w)[0]
    for off in (-1, 1):   # N itself is not stored anywhere: the gate on dL/dp tells N from N +- 1 at this size
        assert not B.check_loss_gradient((dp * n / (n + off)).astype(np.float32), p, t, w)[0], off
    # the other branch: every weighted error zero -> the mean over all elements (N = numel), gradient 2 w (p - t) / numel = 0
    loss0, dp0, n0, masked0 = B.weighted_mse(p, np.where(w > 0, p, t), w)
    assert loss0 == 0 and not masked0 and n0 == w.size and not dp0.any()


def test_adam_without_bias_correction_is_refused():
    rng = np.random.default_rng(3)
    n = 4096
    p0 = rng.standard_normal(n).astype(np.float32)
    m0 = np.zeros(n, np.float32)
    v0 = np.zeros(n, np.float32)
    for t in (1, 2, 3):
        g = (rng.standard_normal(n) * 1e-3).astype(np.float32)
        sc = B.adam_scalars(1e-3, 0.9, 0.999, 1e-8, t)
        rm, rv = B.adam_moments(g, m0, v0, sc, 0.5)
        m1, v1 = rm.astype(np.float32), rv.astype(np.float32)
        p1 = (p0 + B.adam_update(m1, v1, sc)).astype(np.float32)
        assert B.check_adam(p0, g, m0, v0, p1, m1, v1, sc, 0.5) == (True, True, True), t
        bad = (p0 + B.adam_update(m1, v1, sc, bias_correction=False)).astype(np.float32)
        assert not B.check_adam(p0, g, m0, v0, bad, m1, v1, sc, 0.5)[2], t
        assert not B.check_adam(p0, g, m0, v0, p1, m1, v1, sc, 1.0)[0], "grad_scale ignored"
        p0, m0, v0 = p1, m1, v1


def test_f32_moments_cannot_hold_a_bound_relative_to_m():
    """Why adam_kernel forms its moments in double: m = b1 m + (1 - b1) g formed in f32 rounds each term on its own, and where the new
    gradient opposes the old moment the sum is small beside them -- no f32 form holds 4 * 2^-24 relative to m there.  The same
    values through double, rounded once, hold 2^-24."""
    rng = np.random.default_rng(11)
    n = 1 << 16
    m0 = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    g = (-9.0 * m0 * (1 + 1e-3 * rng.standard_normal(n))).astype(np.float32)       # (1 - b1) g ~ -b1 m
    sc = B.adam_scalars(1e-3, 0.9, 0.999, 1e-8, 2)
    rm, _ = B.adam_moments(g, m0, np.zeros(n, np.float32), sc, 0.5 * 2)
    f = np.float32
    m_f32 = f(sc["b1"]) * m0 + (f(1) - f(sc["b1"])) * (g * f(1.0))
    rel = np.abs(m_f32.astype(np.float64) - rm) / np.abs(rm)
    i = int(np.argmax(rel))
    print(f"f32 moments: element {i}: old term {sc['b1'] * m0[i]:.9g} new term {(1 - sc['b1']) * g[i]:.9g} exact {rm[i]:.9g} f32 {m_f32[i]:.9g}: "
          f"{rel[i] / B.U:.0f} * 2^-24 relative; {int((rel > 4 * B.U).sum())} of {n} elements above 4 * 2^-24")
    assert rel.max() > 4 * B.U
    assert (np.abs(rm.astype(np.float32).astype(np.float64) - rm) <= B.U * np.abs(rm)).all()
