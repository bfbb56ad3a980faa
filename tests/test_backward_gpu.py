"""Per-launch parity of the training backward pass (csrc/train.hip and the train_*.hip files it walks): after ONE Trainer.forward_backward per case and arithmetic
the plan is walked in reverse and every step's result is compared with a float64 computation of that one operation on the
tensors AS THE DEVICE HOLDS THEM (tests/bwd_ref.py): forward activations from Model.debug_activation, gradients from
Trainer.debug_tensor, parameters and their gradients from Trainer.read, what ran from Trainer.backward_steps.  Needs an MI355X.

Bit-equal: the padded masked gradient dY [Y > 0] with its zero border; the counts of non-zero values in padding channels and
  border (0); the split copy (= layer_ref.split_bf16 of the masked gradient, and hi + lo); the scatter of the concat-input
  gradient; the max-pool backward (first maximum); the gradient of a tensor with two consumers (pool and skip) as float32 of
  the sum of the two device contributions; the mask of dL/dp.  N of the loss is stored nowhere: dL/dp is held to 4 * 2^-24 of
  the reference's N, which refuses N +- 1 at these sizes (tests/test_backward_cpu.py).
Derived bounds (bwd_ref): upsampling backward (n + 3) 2^-24 T(|dout|), n = the largest number of outputs feeding one input
  (per axis 2 f, 1 for factor 1); head dz (cout + 4) 2^-24 sum |terms| per head -- two heads add into one dz, the second `+=`
  rounds the total once more: 2^-24 sum |terms| on top when there are two --; dL/dp 4 * 2^-24 relative; loss 5 * 2^-24 relative
  per head (one more 2^-24 for the f32 sum of two heads); Adam element-wise, steps 1-3 with grad_scale 0.5.
Weight, bias, head-weight and input gradients: |got - ref| <= g_acc S + g_out |ref|, g_acc = 4 max(e_fmt, e_acc32) from the
  reference alone on a seeded sample (bwd_ref.wgrad_allowances, check_dgrad); g_out = 2^-24, 2^-17 where the input gradient
  is stored as (hi, lo) pairs first.  The range sums of a weight-gradient launch are added by float atomics in an order that
  chance decides: the emulation adds them in three orders and takes the largest error.
The training forward's fused split-bf16 launches get layer_ref's conv gate with the bf16x3 emulation on the same walk.

Cases.  A: the golden nets affs_f4i2, affs_f3i3 (27 -> 81 channels: tile 128 x 32), mtlsd_f4i2 (two heads) with their trained
weights, the family nets 2d_mtlsd_f4i2 ((1,3,3) kernels, (1,2,2) pooling, ten sections) and from_2d_mtlsd_f3i2 (12 input
channels), each at the smallest input its net admits, every element.  C: the 12 / 60 / 300 net at bwd_ref.C_SHAPE (ragged: see
there; Wo % 8 in {1, 7} is possible only at the bottom level, the upper levels have Wo % 8 in {2, 6}).  D: the full-width
12 x 5^3 net at (29, 100, 100), weight gradients on sampled (n, c) pairs with all taps and voxels, the rest in full.  Branches:
the two-head net with one head's targets equal to its predictions where w > 0 (the loss's all-elements branch), an all-zero
weights head, and weights that are non-zero only in a corner of the output, so that the output gradients hold exact zeros and
both upsampling forms take their g == 0 skips.  Arithmetics f32, split-bf16, each also deterministic, in this process; one
child process per development knob set to 0 runs affs_f3i3 and case C.

KX = 2 instantiations (wgrad_kernel<2>, wgrad_tiled_kernel<2>) are unreached: Model has no x-width-2 kernel.

Records (BACKWARD-FORM lines): largest err / S per arithmetic and form on the MI355X with the largest gate of those launches, over
every case and knob child, deterministic runs folded into their arithmetic (the full table is in DESIGN.md section 4, Training):

  arithmetic   form                                                largest err / S      largest g_acc
  f32          input gradient f32 (/ split-K)                      1.39e-05 / 4.61e-06  4.03e-05 / 4.25e-05
  f32          weight gradient wave-f32 KX 1 / KX 3                1.76e-05 / 4.42e-05  7.61e-05 / 1.77e-04
  f32          weight gradient tiled-f32 KX 1 / KX 3               5.93e-06 / 2.12e-05  3.61e-05 / 8.40e-05
  f32          bias sums, head weights                             1.49e-06, 1.03e-06   1.79e-04, 8.43e-06
  split-bf16   input gradient split-bf16 raw (/ split-K)           2.25e-05 / 1.98e-05  8.93e-05 / 7.91e-05
  split-bf16   input gradient split-bf16 converted (/ split-K)     3.09e-05 / 2.90e-05  8.09e-05 / 7.67e-05
  split-bf16   training forward, fused split launch                3.69e-05             7.62e-05
  split-bf16   weight gradient split-bf16 KX 1, six tiles          1.31e-05 .. 2.40e-05 8.79e-05
  split-bf16   weight gradient split-bf16 KX 3, six tiles          1.98e-05 .. 2.64e-05 2.25e-04
  split-bf16   bias sums fused / colsum                            9.91e-06 / 7.63e-06  1.69e-04 / 1.72e-04
  both         upsampling backward scatter / gather, err / bound   0.36 / 0.36          1
Wall time of this file on the MI355X: 3 min 43 s (39 tests; case D 13 to 21 s per arithmetic, a knob child 9 to 17 s, every other
test under 9 s).  Case D's weight gradients are sampled with bwd_ref.WGRAD_SAMPLE = 2 048 output elements per launch.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bwd_ref as B  # noqa: E402
import layer_ref as L  # noqa: E402

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, os.cpu_count() or 1))

U = B.U
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
ARITHMETICS = ["f32", "split-bf16", "f32+deterministic", "split-bf16+deterministic"]
KNOBS = ["BSMI_WGRAD_X3", "BSMI_DGRAD_X3", "BSMI_FWD_X3", "BSMI_DGRAD_RAW", "BSMI_TRAIN_FUSE_COLSUM", "BSMI_TRAIN_WSTREAM", "BSMI_PACK_T"]
D_SHAPE = (29, 100, 100)


# ---- nets ---------------------------------------------------------------------------------------------------------------------
def case_net(tag):
    """(net config, state dict, in_shape) of a case"""
    if tag == "C":
        from bootstrapper_amd.synth import synthetic_state_dict
        return B.C_NET, synthetic_state_dict(B.C_NET, 3), B.C_SHAPE
    if tag == "D":
        from bootstrapper_amd.synth import synthetic_state_dict
        from test_lib_cpu import AFFS_NET_CONFIG
        return AFFS_NET_CONFIG, synthetic_state_dict(AFFS_NET_CONFIG, 0), D_SHAPE
    if tag in ("affs_f4i2", "affs_f3i3", "mtlsd_f4i2"):
        from test_train_gpu import _net_config
        d = np.load(os.path.join(GOLDEN_DIR, "train_affs_f3i3_lr1e-2.npz" if tag == "affs_f3i3" else f"train_{tag}.npz"))
        meta = json.loads(bytes(d["config"]).decode())
        nc = _net_config(meta)
        return nc, {k[3:]: d[k] for k in d.files if k.startswith("w0:")}, B.smallest_shape(nc, meta["in_shape"])
    from test_oracle_unet import family_case
    nc, sd, ins, _, _ = family_case(GOLDEN_DIR, tag)
    good = tuple(ins[0].shape[-3:]) if len(nc["downsample_factors"][0]) == 3 else (10,) + tuple(ins[0].shape[-2:])
    shape = B.smallest_shape(nc, good)
    return nc, sd, (shape if len(nc["downsample_factors"][0]) == 3 else (10,) + shape[1:])   # a 2-D setup trains ten sections per step


def step_inputs(ops, seed=0, corner_only=()):
    """x (D, H, W, Cin) in [-1, 1), per head binary targets and weights (a fifth zero) as (M, cout) arrays.  corner_only: heads whose
    weights are non-zero only in a 2 x 2 corner of the output."""
    rng = np.random.default_rng(seed)
    x = (rng.random(ops[0]["shape"], dtype=np.float32) * 2 - 1).astype(np.float32)
    ts, ws = [], []
    for o in ops:
        if o["type"] != "head":
            continue
        d, h, w_, c = o["shape"]
        ts.append((rng.random((d * h * w_, c)) > 0.5).astype(np.float32))
        w = rng.random((d * h * w_, c)).astype(np.float32)
        w[rng.random(w.shape) < 0.2] = 0
        if len(ts) - 1 in corner_only:
            keep = np.zeros((d, h, w_), dtype=bool)
            keep[:, :2, :2] = True
            w[~keep.ravel()] = 0
        ws.append(w)
    return x, ts, ws


def _cuda_cl(a, shape):
    """(M, C) or (D, H, W, C) host array -> contiguous CUDA (C, D, H, W)"""
    return torch.from_numpy(np.ascontiguousarray(a.reshape(tuple(shape[:3]) + (-1,)).transpose(3, 0, 1, 2))).cuda()


# ---- records --------------------------------------------------------------------------------------------------------------------
class Record:
    """largest err / S and the largest gate it met, per (arithmetic, form); what the launches were, for the coverage test"""

    def __init__(self):
        self.forms, self.seen = {}, set()

    def add(self, arith, form, es, g_acc):
        old = self.forms.get((arith, form), (0.0, 0.0))
        self.forms[(arith, form)] = (max(old[0], es), max(old[1], g_acc))

    def lines(self):
        return [f"BACKWARD-FORM {json.dumps([a, f, es, g])}" for (a, f), (es, g) in sorted(self.forms.items())] + \
               [f"BACKWARD-SEEN {json.dumps(sorted(self.seen))}"]


RECORD = Record()


def _wform(w):
    return f"wgrad {w['family']} KX {w['kx']} tile {w['tile'][0]}x{w['tile'][1]}"


def note_coverage(rec, bsteps, arith):
    for b in bsteps:
        if b["type"] == "up":
            rec.seen.add(f"up {b['up']}")
        if b["type"] != "conv":
            continue
        rec.seen.add(f"bias {b['bias']}")
        if b["fwd_split"]:
            rec.seen.add("forward split-bf16")
        for w in b["wgrad"]:
            rec.seen.add(_wform(w) if w["family"] == "split-bf16" else f"wgrad {w['family']} KX {w['kx']}")
            if w["det_workspace"] and w["ranges"] > 1:
                rec.seen.add("wgrad deterministic workspace, several ranges")
            if w["cbase"] > 0:
                rec.seen.add("wgrad second slot")
        d = b["dgrad"]
        if d:
            rec.seen.add(f"dgrad {d['arithmetic']}")
            for k in ("raw", "converted", "split_k", "scatter", "residual"):
                if d[k]:
                    rec.seen.add(f"dgrad {k}")


# ---- one case -------------------------------------------------------------------------------------------------------------------
def run_case(case, nc, sd, shape, arith, record=RECORD, sampled=False, seed=0, corner_only=(), retarget=(), zero_weights=()):
    """One forward_backward of the net in `arith`, then every step of the backward pass against its reference.  retarget: heads
    whose targets are set to the device's own predictions wherever w > 0 (after a first step that produces them);
    zero_weights: heads whose weights are all zero.  -> dict of facts about the run (for the branch tests)."""
    from bootstrapper_amd.unet import Model
    from bootstrapper_amd.training import Trainer
    from test_layers_gpu import _check_conv, Record as FwdRecord
    t_start = time.time()
    arithmetic, det = arith.split("+")[0], arith.endswith("+deterministic")
    prec = "bf16x3" if arithmetic == "split-bf16" else "f32"
    ops = L.walk(nc, shape)
    x, ts, ws = step_inputs(ops, seed, corner_only)
    for h in zero_weights:
        ws[h][:] = 0
    heads = [i for i, o in enumerate(ops) if o["type"] == "head"]
    m = Model(nc, precision="f32").load_state_dict(sd)
    tr = Trainer(m, shape, lr=1e-3, arithmetic=arithmetic, deterministic=det)
    raw = _cuda_cl(x, ops[0]["shape"])
    to_dev = lambda arrs: [_cuda_cl(a, ops[h]["shape"]) for a, h in zip(arrs, heads)]
    if retarget:
        tr.forward_backward(raw, to_dev(ts), to_dev(ws))
        for h in retarget:
            p = list(tr.predictions().values())[h].cpu().numpy().reshape(ts[h].shape[1], -1).T
            ts[h] = np.where(ws[h] > 0, p, ts[h]).astype(np.float32)
    loss = tr.forward_backward(raw, to_dev(ts), to_dev(ws))
    plan = m.plan_steps()
    L.check_walk(ops, plan)
    bsteps = tr.backward_steps()
    note_coverage(record, bsteps, arith)
    assert all(b["deterministic"] == det for b in bsteps)
    rng = np.random.default_rng(4321)
    facts = dict(loss=loss, zero_dout_up=0, masked=[], bsteps=bsteps)

    acts = [None if o["type"] == "head" else m.debug_activation(i) for i, o in enumerate(ops)]
    preds = [t.cpu().numpy().reshape(t.shape[0], -1).T for t in tr.predictions().values()]   # (M, cout) per head
    shapes = tr.param_shapes()
    par = {k: tr.read(k).reshape(shapes[k]) for k in shapes}
    grd = {k: tr.read(k, "grad").reshape(shapes[k]) for k in shapes}
    assert all(np.isfinite(g).all() for g in grd.values())
    cons = B.consumers(ops)
    douts, gps, gsplits = {}, {}, {}

    def dout(i):
        if i not in douts:
            douts[i] = tr.debug_tensor(i, "dout")
        return douts[i]

    def where(i):
        o = ops[i]
        extra = f" {o['prefix']} conv {o['conv']}" if o["type"] == "conv" else ""
        return f"{case} {arith} step {i} ({o['type']}{extra}, shape {o['shape']})"

    # -- the training forward's fused split launches: layer_ref's conv gate with the bf16x3 emulation
    fwd_rec = FwdRecord()
    for i, o in enumerate(ops):
        if o["type"] == "conv" and bsteps[i]["fwd_split"]:
            p = dict(plan[i], form="gather", flags=())
            _check_conv(case, "bf16x3", i, o, p, acts[i], par, lambda s: L.Dense(acts[s]), None, sampled, rng, fwd_rec, where, plan)
    for (_, _, _), (es, g) in fwd_rec.forms.items():
        record.add(arith, "forward fused split-bf16", es, g)

    # -- loss and dL/dp, from the device's own predictions
    ref_losses = []
    for h, i in enumerate(heads):
        l, _, n, masked = B.weighted_mse(preds[h], ts[h], ws[h])
        ref_losses.append(l)
        facts["masked"].append(masked)
        dp = tr.debug_tensor(i, "head_dp").reshape(-1, ops[i]["shape"][3])
        ok, _, _ = B.check_loss_gradient(dp, preds[h], ts[h], ws[h])
        assert ok, f"{where(i)}: dL/dp (N = {n}, masked {masked})"
    ref_loss = sum(ref_losses)
    tol = 5 * U * sum(abs(l) for l in ref_losses)     # four roundings per head (d, d d, w ., the cast); the fifth covers the f32 sum of two heads
    print(f"{case} {arith}: loss {loss!r} reference {ref_loss!r} (gate {tol:.3e})")
    assert abs(loss - ref_loss) <= tol, (loss, ref_loss, tol)

    for i in range(len(ops) - 1, -1, -1):
        o = ops[i]
        kinds = sorted(k for _, k, _ in cons[i])
        # ---- the gradient of this step's output, from its consumers
        if o["type"] in ("conv", "pool", "up"):
            got = dout(i)
            assert got.shape == tuple(o["shape"]) and np.isfinite(got).all(), where(i)
            if kinds == ["conv"]:
                pass                                    # the consumer's input-gradient launch wrote it: checked there
            elif kinds and set(kinds) == {"head"}:
                _check_head_dz(where(i), ops, cons[i], heads, acts[i], preds, tr, par, grd, got, record, arith)
            elif kinds == ["up"]:
                j = cons[i][0][0]
                ok, nbad, ratio = B.check_upsample_backward(got, dout(j), o["shape"], ops[j]["factor"], ops[j]["offset"])
                record.add(arith, f"up {bsteps[j]['up']} (err / bound)", ratio, 1.0)
                facts["zero_dout_up"] += int(np.count_nonzero(dout(j) == 0))
                assert ok, f"{where(i)}: upsampling backward ({bsteps[j]['up']}): {nbad} elements off, largest err / bound {ratio:.3f}"
            elif kinds in (["cat"], ["cat", "pool"]):
                parts = []
                for j, k, sl in cons[i]:
                    if k == "pool":
                        parts.append(B.maxpool_backward(acts[i], dout(j), ops[j]["factor"]))
                    else:
                        dcat = tr.debug_tensor(j, "dcat")
                        slots = [(org, c) for _, org, c in ops[j]["src"]]
                        parts.append(B.scatter(dcat, slots, [ops[s]["shape"] for s, _, _ in ops[j]["src"]])[sl])
                want = parts[0] if len(parts) == 1 else (parts[0].astype(np.float64) + parts[1].astype(np.float64)).astype(np.float32)
                assert np.array_equal(got, want), f"{where(i)}: {kinds} not bit-equal, {int((got != want).sum())} elements differ"
            elif kinds == ["pool"]:
                assert np.array_equal(got, B.maxpool_backward(acts[i], dout(cons[i][0][0]), ops[cons[i][0][0]]["factor"])), where(i)
            else:
                raise AssertionError(f"{where(i)}: consumers {kinds} not handled")
        if o["type"] != "conv":
            continue
        # ---- a conv step: masking, split copy, bias, weight and input gradients
        b = bsteps[i]
        ks, first = B.pass_kernels(ops, i)
        ci, last = o["conv"], o["conv"] == len(ks) - 1
        P = B.border_of(ks, ci)
        assert tuple(b["border"]) == P, (where(i), b["border"], P)
        gp = tr.debug_tensor(i, "gmask")
        gps[i] = gp
        assert B.check_masked(gp, dout(i), acts[i], P), f"{where(i)}: masked padded gradient not bit-equal (border non-zeros {B.border_nonzero(gp, P)})"
        assert not tr.debug_tensor(i, "pad_count").any(), f"{where(i)}: non-zero padding channels / border {tr.debug_tensor(i, 'pad_count')}"
        if b["has_split"]:
            hi, lo = tr.debug_tensor(i, "gsplit_hi"), tr.debug_tensor(i, "gsplit_lo")
            assert B.check_split(hi, lo, gp), f"{where(i)}: split copy of the masked gradient"
            gsplits[i] = tr.debug_tensor(i, "gsplit")
            assert np.array_equal(gsplits[i], hi + lo), where(i)
        g = B.interior(gp, P)
        key = f"{o['prefix']}.conv_pass.{2 * ci}"
        for bk in [key + ".bias"] + ([o["prefix"] + ".residual.0.bias"] if last else []):
            ok, worst, g_acc = B.check_bias(grd[bk], g, rng)
            record.add(arith, f"bias {b['bias']}", worst["max_err_over_S"], g_acc)
            assert ok, f"{where(i)}: {bk} ({b['bias']}): {worst}"
        launches = [(False, sl) for sl in range(len(o["src"]))] + ([(True, sl) for sl in range(len(o["res"]))] if last else [])
        assert len(b["wgrad"]) == len(launches), (where(i), b["wgrad"])
        for (residual, sl), w in zip(launches, b["wgrad"]):
            srcs, kernel = (o["res"], (1, 1, 1)) if residual else (o["src"], o["kernel"])
            s, org, c = srcs[sl]
            cbase = sum(cc for _, _, cc in srcs[:sl])
            assert (w["residual"], w["n"], w["c"], w["cbase"]) == (residual, o["shape"][3], c, cbase), (where(i), w)
            assert w["kx"] == kernel[2] and w["ranges"] * w["lines_per_range"] >= o["shape"][0] * o["shape"][1] > (w["ranges"] - 1) * w["lines_per_range"]
            xin = B.crop(acts[s], org, tuple(o["shape"][d] + kernel[d] - 1 for d in range(3)))
            gw = B.w5(grd[(o["prefix"] + ".residual.0" if residual else key) + ".weight"])
            gw = gw.reshape(gw.shape[0], gw.shape[1], -1)[:, cbase:cbase + c]
            if sampled:
                n_idx, c_idx = B.wgrad_sample(gw.shape[0], c, gw.shape[2], w["tile"][0], w["tile"][1], rng, live_n=B.live_channels(g), live_c=B.live_channels(xin))
                ok, worst, g_acc, e_fmt, e_acc = B.check_wgrad(gw[n_idx][:, c_idx], g, xin, kernel, w, rng, n_idx, c_idx, full=False)
            else:
                ok, worst, g_acc, e_fmt, e_acc = B.check_wgrad(gw, g, xin, kernel, w, rng)
            record.add(arith, _wform(w) + (" det" if w["det_workspace"] else ""), worst["max_err_over_S"], g_acc)
            print(f"{where(i)}: {_wform(w)} {'residual ' if residual else ''}slot {sl} ranges {w['ranges']} x {w['lines_per_range']} lines: "
                  f"max err/S {worst['max_err_over_S']:.3e}, g_acc {g_acc:.3e} (e_fmt {e_fmt:.3e}, e_acc32 {e_acc:.3e})")
            assert ok, f"{where(i)}: {_wform(w)} {'residual ' if residual else ''}slot {sl} (row = n, channel = c * ntap + tap): {worst}"
        d = b["dgrad"]
        if ops[o["src"][0][0]]["type"] == "input":
            assert d is None, where(i)
            continue
        assert d is not None and d["scatter"] == (ci == 0) and d["residual"] == (ci == 0 and len(ks) > 1), (where(i), d)
        assert d["arithmetic"] == ("split-bf16" if b["has_split"] else "f32"), (where(i), d)
        held = gsplits if b["has_split"] else gps      # a split-bf16 launch reads the split copies (verified above), not the f32 tensors
        res = None
        if d["residual"]:
            j = first + len(ks) - 1
            res = (held[j], B.border_of(ks, len(ks) - 1), B.pass_crop(ks), B.w5(par[o["prefix"] + ".residual.0.weight"]))
        stage = B.dgrad_stage(held[i], P, o["kernel"], B.w5(par[key + ".weight"]), res)
        got = tr.debug_tensor(i, "dcat") if ci == 0 else dout(o["src"][0][0])
        dprec = "bf16x3" if d["arithmetic"] == "split-bf16" else "f32"
        g_out = 2.0 ** -17 if d["converted"] else U
        ok, worst, cv, g_acc, e_fmt, e_acc, es = B.check_dgrad(got, stage, dprec, d["split_k"], g_out, rng)
        form = f"dgrad {d['arithmetic']}{' raw' if d['raw'] else ''}{' converted' if d['converted'] else ''}{' split-k' if d['split_k'] else ''}"
        record.add(arith, form, es, g_acc)
        print(f"{where(i)}: {form} BN {d['bn']} {d['ksteps']} K-steps: max err/S {es:.3e}, g_acc {g_acc:.3e} (e_fmt {e_fmt:.3e}, e_acc32 {e_acc:.3e})")
        assert ok, f"{where(i)}: {form}: {L.describe(worst, cv, got.shape)}"
    tr.close()
    del m
    print(f"{case} {arith}: {len(ops)} steps checked in {time.time() - t_start:.1f} s")
    return facts


def _check_head_dz(where, ops, cons_i, heads, z, preds, tr, par, grd, got_dz, record, arith):
    """dz of the last trunk activation (every head adds into it) and each head's weight and bias gradients"""
    M = z.shape[0] * z.shape[1] * z.shape[2]
    z2 = z.reshape(M, -1)
    ref, bound, T_all = 0.0, 0.0, 0.0
    for j, _, _ in cons_i:
        h, pre = heads.index(j), ops[j]["prefix"]
        dp = tr.debug_tensor(j, "head_dp").reshape(M, -1)
        wc, wr = (par[f"{pre}.{k}.0.weight"].reshape(dp.shape[1], -1) for k in ("conv_pass", "residual"))
        dz, T, dW, SW, db, Sb, dl = B.head_backward(z2, preds[h], dp, wc, wr)
        ref = ref + dz
        bound = bound + (dp.shape[1] + 4) * U * T
        T_all = T_all + T
        # weight and bias gradients: exact f32 products (e_fmt = 0); the allowance from an f32 emulation in voxel order
        p32, dp32 = preds[h].astype(np.float32), dp.astype(np.float32)
        dl32 = (dp32 * p32) * (np.float32(1) - p32)
        z32 = z2.astype(np.float32)
        hrng = np.random.default_rng(99)
        eW = max(B.reduction_allowance(dl32[:, o:o + 1] * z32, dW[o], SW[o], hrng) for o in range(dp.shape[1]))
        gW, gb = L.gate(0.0, eW), L.gate(0.0, B.reduction_allowance(dl32, db, Sb, hrng))
        for k in ("conv_pass", "residual"):
            ok, worst = L.compare(grd[f"{pre}.{k}.0.weight"].reshape(dW.shape).astype(np.float64), dW, SW, gW, U)
            record.add(arith, "head weights", worst["max_err_over_S"], gW)
            assert ok, f"{where}: {pre}.{k}.0.weight: {worst}"
            ok, worst = L.compare(grd[f"{pre}.{k}.0.bias"].astype(np.float64)[None], db[None], Sb[None], gb, U)
            assert ok, f"{where}: {pre}.{k}.0.bias: {worst}"
    # (cout + 4) has no spare: Wc + Wr rounds once, dlogit = (dp p)(1 - p) three times, each of the cout fmas once.  The first head
    # adds into zeros (exact); every later head's `+=` rounds the total once more
    bound = bound + (len(cons_i) - 1) * U * T_all
    err = np.abs(got_dz.reshape(M, -1).astype(np.float64) - ref)
    bad = err > bound
    assert not bad.any(), f"{where}: head dz: {int(bad.sum())} elements off, first {tuple(int(v[0]) for v in np.nonzero(bad))}, err {err[bad][0]:.3e} bound {bound[bad][0]:.3e}"


# ---- the default rule, in this process ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHMETICS)
@pytest.mark.parametrize("tag", ["affs_f4i2", "affs_f3i3", "mtlsd_f4i2", "2d_mtlsd_f4i2", "from_2d_mtlsd_f3i2"])
def test_case_a_golden_and_family_nets(tag, arith):
    run_case(f"A:{tag}", *case_net(tag), arith)


@pytest.mark.parametrize("arith", ARITHMETICS)
def test_case_c_12_60_300_channels_ragged(arith):
    """... and the shape keeps the properties the case exists for, read from what the device says it launched"""
    nc, sd, shape = case_net("C")
    facts = run_case("C", nc, sd, shape, arith)
    ops = L.walk(nc, shape)
    convs = [(o, b) for o, b in zip(ops, facts["bsteps"]) if o["type"] == "conv"]
    rag8 = {o["shape"][3]: o["shape"][2] % 8 for o, _ in convs if o["shape"][2] % 8 in (1, 2, 6, 7)}
    assert set(rag8) == {12, 60, 300} and rag8[300] in (1, 7), rag8
    assert all(o["shape"][1] != o["shape"][2] for o, _ in convs)
    launches = [(o, w) for o, b in convs for w in b["wgrad"]]
    if arith == "f32+deterministic":
        assert all(w["ranges"] == 1 for _, w in launches)   # one workgroup per element: nothing to order
    else:
        assert any((o["shape"][0] * o["shape"][1]) % w["lines_per_range"] for o, w in launches), "no launch with a short last line range"
    if arith == "split-bf16+deterministic":
        assert any(w["det_workspace"] and w["ranges"] == 32 and o["shape"][0] * o["shape"][1] > 32 for o, w in launches)
    if arith.startswith("split-bf16"):
        tiles = {(w["tile"], w["kx"]) for _, w in launches}
        assert {t for t, _ in tiles} >= {(32, 32), (32, 64), (64, 32), (64, 64), (128, 64)} and {k for _, k in tiles} == {1, 3}, tiles
    assert any(w["cbase"] > 0 for _, w in launches)


@pytest.mark.parametrize("arith", ["f32", "split-bf16", "split-bf16+deterministic"])
def test_case_d_full_width_net(arith):
    facts = run_case("D", *case_net("D"), arith, sampled=True)
    assert any(w["n"] == 1500 and w["c"] == 1500 for b in facts["bsteps"] if b["type"] == "conv" for w in b["wgrad"])


@pytest.mark.parametrize("arith", ["split-bf16", "split-bf16+deterministic"])
def test_branches_of_loss_and_upsampling(arith):
    """Run 1: head 0's targets equal its predictions where w > 0 (every weighted error zero: the mean over all elements, a zero
    gradient), head 1's weights non-zero only in a corner, so the output gradients hold exact zeros and the upsampling backward
    (scatter form, gather form when deterministic) takes its g == 0 skips.  Run 2: head 1's weights all zero."""
    nc, sd, shape = case_net("mtlsd_f4i2")
    f1 = run_case("branches:1", nc, sd, shape, arith, retarget=(0,), corner_only=(1,))
    assert f1["masked"] == [False, True] and f1["zero_dout_up"] > 0, (f1["masked"], f1["zero_dout_up"])
    f2 = run_case("branches:2", nc, sd, shape, arith, zero_weights=(1,))
    assert f2["masked"] == [True, False]


@pytest.mark.parametrize("arith", ["f32", "split-bf16"])
def test_adam_three_steps_with_gradient_scale(arith):
    """Element-wise from the device's own p, g, m, v before each of three steps with grad_scale = 0.5; the 4-float padding
    entries of the flat buffers stay 0."""
    import ctypes as C
    from bootstrapper_amd.unet import Model
    from bootstrapper_amd.training import Trainer
    from bootstrapper_amd._lib import lib, check
    nc, sd, shape = case_net("affs_f3i3")
    ops = L.walk(nc, shape)
    x, ts, ws = step_inputs(ops, 1)
    heads = [i for i, o in enumerate(ops) if o["type"] == "head"]
    m = Model(nc, precision="f32").load_state_dict(sd)
    tr = Trainer(m, shape, lr=1e-3, arithmetic=arith)
    keys = list(tr.param_shapes())
    real = np.zeros(tr.params.numel(), dtype=bool)
    for k in keys:
        off, cnt = C.c_uint64(), C.c_uint64()
        check(lib.bsmi_unet_train_param_info(m._h, k.encode(), C.byref(off), C.byref(cnt)))
        real[off.value:off.value + cnt.value] = True
    assert (~real).any(), "no padding entries in this net's flat buffers"
    read = lambda what: np.concatenate([tr.read(k, what) for k in keys])
    for t in (1, 2, 3):
        tr.forward_backward(_cuda_cl(x, ops[0]["shape"]), [_cuda_cl(a, ops[h]["shape"]) for a, h in zip(ts, heads)],
                            [_cuda_cl(a, ops[h]["shape"]) for a, h in zip(ws, heads)])
        p0, g, m0, v0 = read("param"), read("grad"), read("exp_avg"), read("exp_avg_sq")
        check(lib.bsmi_unet_train_adam_step(m._h, tr.lr, tr.betas[0], tr.betas[1], tr.eps, 0.5, tr._stream()))
        torch.cuda.synchronize()
        assert tr.step_count() == t
        sc = B.adam_scalars(tr.lr, tr.betas[0], tr.betas[1], tr.eps, t)
        oks = B.check_adam(p0, g, m0, v0, read("param"), read("exp_avg"), read("exp_avg_sq"), sc, 0.5)
        assert oks == (True, True, True), (arith, t, oks)
        assert not tr.params.cpu().numpy()[~real].any() and not tr.grads.cpu().numpy()[~real].any(), t
    tr.close()


# ---- the development knobs, a child process each --------------------------------------------------------------------------------------
_SEEN = {}
_STOP = []            # a child ended on a signal or a timeout: no further GPU work in this run
_DEAD = (134, 139, 124, 137, -6, -11, -9)


@pytest.mark.parametrize("knob", KNOBS)
def test_thinned_cases_with_knob_off(knob, tmp_path):
    """affs_f3i3 and case C with one development knob set to 0 (read once per process): a child process under its own timeout
    that writes a JSON record; a child that dies on a signal or times out fails the test and stops the remaining ones."""
    assert not _STOP, f"a child process died earlier ({_STOP[0]}): no further GPU work in this run"
    out = str(tmp_path / "record.json")
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), knob, out], env=dict(os.environ, **{knob: "0"}), capture_output=True,
                           text=True, timeout=600, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _STOP.append(f"{knob}=0: timeout")
        raise
    if r.returncode in _DEAD or r.returncode < 0:
        _STOP.append(f"{knob}=0: exit status {r.returncode}")
    assert r.returncode == 0, f"{knob}=0:\n" + r.stdout[-6000:] + r.stderr[-3000:]
    with open(out) as f:
        rec = json.load(f)
    assert rec["cases"] and rec["forms"], rec
    for line in rec["forms"]:
        print("BACKWARD-FORM", json.dumps([f"{knob}=0"] + line))
    for k in rec["seen"]:
        _SEEN.setdefault(k, f"{knob}=0")
    expect_absent = {"BSMI_WGRAD_X3": "wgrad split-bf16", "BSMI_DGRAD_X3": "dgrad split-bf16", "BSMI_FWD_X3": "forward split-bf16",
                     "BSMI_DGRAD_RAW": "dgrad raw", "BSMI_TRAIN_FUSE_COLSUM": "bias fused"}.get(knob)
    if expect_absent:
        assert not [k for k in rec["seen"] if k.startswith(expect_absent)], (knob, rec["seen"])


ALL_FORMS = ([f"wgrad split-bf16 KX {kx} tile {tn}x{tc}" for kx in (1, 3) for tn in (32, 64, 128) for tc in (32, 64)] +
             [f"wgrad {fam} KX {kx}" for fam in ("wave-f32", "tiled-f32") for kx in (1, 3)] +
             ["dgrad f32", "dgrad split-bf16", "dgrad raw", "dgrad converted", "dgrad scatter", "dgrad residual", "up scatter", "up gather",
              "bias fused", "bias colsum", "wgrad deterministic workspace, several ranges", "wgrad second slot", "forward split-bf16"])


def test_every_backward_form_was_reached():
    """The union over this module's run -- the four arithmetics in this process, the knob children -- covers every form
    bsmi_unet_train_debug_step_info can report for the listed nets.  Unreached by construction: the KX = 2 instantiations (no
    x-width-2 kernel in Model).  (last in the module: it needs the tests above to have run)"""
    assert not _STOP, f"a child process died earlier ({_STOP[0]})"
    seen = dict(_SEEN)
    for k in RECORD.seen:
        seen.setdefault(k, "default rule")
    for line in RECORD.lines():
        print(line)
    print({k: seen.get(k) for k in ALL_FORMS + ["dgrad split_k"]})
    missing = [k for k in ALL_FORMS if k not in seen]
    assert not missing, f"no case reached {missing}"


# ---- child process ----------------------------------------------------------------------------------------------------------------
def _main(knob, out):
    rec = Record()
    cases = []
    ariths = ["split-bf16"] + (["f32"] if knob in ("BSMI_TRAIN_FUSE_COLSUM", "BSMI_TRAIN_WSTREAM") else [])
    for arith in ariths:
        for tag in ("affs_f3i3", "C"):
            run_case(tag, *case_net(tag), arith, record=rec)
            cases.append([tag, arith])
    with open(out, "w") as f:
        json.dump({"cases": cases, "forms": [[a, fm, es, g] for (a, fm), (es, g) in sorted(rec.forms.items())], "seen": sorted(rec.seen)}, f)


if __name__ == "__main__":
    _main(sys.argv[1], sys.argv[2])
