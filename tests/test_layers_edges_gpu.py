"""Case E of the per-launch parity of the forward (tests/test_layers_gpu.py holds cases A - D): nets whose channel counts sit on the
edges of the launchers' tile and padding rules (tests/edge_nets.py), every element of every materialised step against float64,
three precisions.  Needs an MI355X.

Gates and comparisons are test_layers_gpu.run_case's, unchanged: |got - ref| <= g_acc S + g_out |ref|, g_acc = 4 max(e_fmt,
e_acc32) from the reference alone (tests/layer_ref.py).  Three kernel variants run E1, E5, E6 and E13 in bf16x3 in a child process
each.  The last test holds the launches of the default rule -- (tile columns BN, N-tiles, exact fit, form, flags) per precision,
from Model.plan_steps() -- to the classes the nets exist for, written out by hand: a rule change that moves a net off its class fails
there, and the net list is revised on purpose.

The head.  G_HEAD of test_layers_gpu is a measured constant from heads of at most 12 input channels; E1 - E13 have up to 64.  Every
head output of case E is held to a bound derived per element from the reference (head_bound): the two f32 fma chains over cin
channels, their biases and their sum give (cin + 4) 2^-24 sum |terms| on the logit; the sigmoid's slope is at most 1 / 4; and
s = 1 / (1 + expf(-y)) in f32 adds 4 * 2^-24 relative to s -- expf within 1 ulp (2 * 2^-24 relative, the documented bound of the
device library's expf; it enters s with the factor e / (1 + e) < 1), one rounding of 1 + e, one of the correctly rounded division,
which is also the rounding of the stored f32 output.  Nets with at most 12 head inputs (E2) keep G_HEAD as well; the others run
run_case with that measured gate lifted, since it was not measured for them.

Largest err / S per (precision, form) over case E on the MI355X with the largest gate of those steps (records, not gates; the
LAYERS-FORM lines, the variant children folded in; also in DESIGN.md section 2, "Case E"):

  precision  form               largest err / S   largest g_acc of those steps
  f32        gather             1.82e-05          4.41e-05
  f32        raster-halo        1.71e-05          4.86e-05
  bf16x3     gather             3.52e-05          7.71e-05
  bf16x3     first-pass         3.12e-05          9.51e-05
  bf16x3     halo-resident      3.00e-05          7.69e-05   (BSMI_H16=2 child)
  bf16x3     winograd F(4x4)    7.44e-05          3.11e-04   (default rule; 3.38e-04 against 1.05e-03 with F(4x4) on every stage)
  bf16       gather             1.53e-02          3.35e-02
  bf16       raster-halo        1.47e-02          2.51e-02
  bf16       box-halo           1.30e-02          2.88e-02
  bf16       first-pass         1.78e-02          4.62e-02
  head (every mode)             1.91e-07 absolute; at most 0.18 of the derived bound (13 inputs), 0.02 at 64 inputs
No step of any net or variant exceeded its gate.
Wall time of this file on the MI355X: 53 s (44 tests; a variant child 7.5 s, E13 in bf16x3 3.5 s, every other case under 2 s).
"""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import edge_nets as E  # noqa: E402
import layer_ref as L  # noqa: E402
import test_layers_gpu as T  # noqa: E402

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, os.cpu_count() or 1))

U = 2.0 ** -24
RECORD = T.Record()
CLASSES = {}          # precision -> {(bn, N-tiles, exact fit, form, flags): net that met it first}
COUTS = {}            # (precision, bn, N-tiles) -> output channel counts met
BELOW_UP = set()      # (precision, cout) of stages that convolve below the upsampling
HEAD_WORST = {}       # head input channels -> largest err / bound
VARIANTS = [("F(4x4) on every stage", {"BSMI_WINO": "2", "BSMI_WINO4": "2"}),
            ("F(2,3) along z on every F(4x4) stage", {"BSMI_WINO_Z": "1"}),
            ("halo-resident form on every narrow stage", {"BSMI_H16": "2"})]


# ---- the head ---------------------------------------------------------------------------------------------------------------
def head_bound(z, w1, b1, w2, b2):
    """(reference, bound) of the head on the rows z (M, cin) float64 as the device holds them: see the module docstring."""
    y = (z @ w1.T + b1) + (z @ w2.T + b2)
    terms = np.abs(z) @ np.abs(w1).T + np.abs(b1) + np.abs(z) @ np.abs(w2).T + np.abs(b2)
    ref = 1.0 / (1.0 + np.exp(-y))
    return ref, (z.shape[1] + 4) * U * terms / 4 + 4 * U * ref


@contextlib.contextmanager
def _head_gate(cin):
    """run_case's measured head gate, kept for heads of at most 12 inputs and lifted for wider ones (check_head holds those)"""
    old = T.G_HEAD
    if cin > 12:
        T.G_HEAD = float("inf")
    try:
        yield
    finally:
        T.G_HEAD = old


def check_plan_and_head(tag, nc, sd, raw, prec):
    """A second forward of the same net: its plan into CLASSES, its head outputs against the derived bound."""
    from bootstrapper_amd.unet import Model
    m = Model(nc, precision=prec).load_state_dict(sd)
    u8, f32 = m.predict_u8(torch.from_numpy(np.ascontiguousarray(raw)).cuda(), want_f32=True)
    torch.cuda.synchronize()
    plan = m.plan_steps()
    ops = L.walk(nc, tuple(raw.shape[-3:]))
    for p in plan:
        if p["type"] != "conv":
            continue
        cout, bn = p["shape"][3], p["bn"]       # (first-pass and box-halo launches have no GEMM tile: BN 0)
        nt = -(-cout // bn) if bn else 0
        CLASSES.setdefault(prec, {}).setdefault((bn, nt, bool(bn) and cout % bn == 0, p["form"], tuple(p["flags"])), tag)
        COUTS.setdefault((prec, bn, nt), set()).add(cout)
        if p["below_up"]:
            BELOW_UP.add((prec, cout))
    for o, p in zip(ops, plan):
        if o["type"] != "head":
            continue
        z = m.debug_activation(o["src"]).astype(np.float64)
        z = z.reshape(-1, z.shape[3])
        pre = o["prefix"]
        w1, b1 = T._w5(sd[pre + ".conv_pass.0.weight"])[:, :, 0, 0, 0].astype(np.float64), sd[pre + ".conv_pass.0.bias"].astype(np.float64)
        w2, b2 = T._w5(sd[pre + ".residual.0.weight"])[:, :, 0, 0, 0].astype(np.float64), sd[pre + ".residual.0.bias"].astype(np.float64)
        ref, bound = head_bound(z, w1, b1, w2, b2)
        got = f32[p["head"]].cpu().numpy().reshape(ref.shape[1], -1).T.astype(np.float64)
        err = np.abs(got - ref)
        ratio = float((err / bound).max())
        HEAD_WORST[z.shape[1]] = max(HEAD_WORST.get(z.shape[1], 0.0), ratio)
        print(f"E:{tag} {prec} head, {z.shape[1]} inputs: max abs err {err.max():.3e}, largest err / bound {ratio:.3f} (bound there "
              f"{bound.ravel()[int((err / bound).argmax())]:.3e})")
        bad = err > bound
        assert not bad.any(), (f"E:{tag} {prec} head: {int(bad.sum())} elements over the derived bound, first (row, channel) "
                               f"{tuple(int(v[0]) for v in np.nonzero(bad))}: err {err[bad][0]:.3e} bound {bound[bad][0]:.3e}")
    del m


def run_edge(tag, prec, record):
    nc, sd, raw = E.edge_case(tag)
    with _head_gate(nc["num_fmaps"]):
        T.run_case(f"E:{tag}", nc, sd, raw, prec, record=record)
    check_plan_and_head(tag, nc, sd, raw, prec)


# ---- the default rule, in this process ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", T.PRECS)
@pytest.mark.parametrize("tag", E.TAGS)
def test_case_e_edge_nets(tag, prec):
    run_edge(tag, prec, RECORD)


def test_a_head_of_more_than_64_inputs_is_refused_before_any_launch():
    """num_fmaps = 65 pads to 80 channels, which the head kernel does not take: bsmi_unet_finalize refuses the net (the forward used
    to run the whole trunk and fail at its last launch), and the handle destroys cleanly."""
    from bootstrapper_amd.synth import synthetic_state_dict
    from bootstrapper_amd.unet import Model
    from bootstrapper_amd._lib import BsmiError, ERR_INVALID
    nc = dict(E.net_config("E1"), num_fmaps=65, fmap_inc_factor=2)
    m = Model(nc, precision="f32")
    with pytest.raises(BsmiError) as ei:
        m.load_state_dict(synthetic_state_dict(nc, 3))
    assert ei.value.code == ERR_INVALID and "head kernel supports at most 64 input channels" in ei.value.msg, ei.value
    raw = torch.zeros(E.SHAPE, dtype=torch.uint8, device="cuda")
    with pytest.raises(BsmiError):          # never finalized: no forward either
        m.predict_u8(raw)
    m.__del__()
    assert not m._h
    # ... and the next net on the device is served as usual
    nc2, sd2, raw2 = E.edge_case("E2")
    out = Model(nc2, precision="f32").load_state_dict(sd2).predict_u8(torch.from_numpy(raw2).cuda())
    torch.cuda.synchronize()
    assert out[0].shape[0] == 6


# ---- the kernel variants, a child process each -----------------------------------------------------------------------------------
_STOP = []            # a child ended on a signal or a timeout: no further GPU work in this run
_DEAD = (134, 139, 124, 137, -6, -11, -9)


def _child(env, timeout):
    import json
    import subprocess
    if _STOP:
        pytest.skip(f"a child process died earlier ({_STOP[0]}): no further GPU work in this run")
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "variant"], env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=timeout, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _STOP.append(f"{env}: timeout after {timeout} s")
        raise
    if r.returncode in _DEAD or r.returncode < 0:
        _STOP.append(f"{env}: exit status {r.returncode}")
    assert r.returncode == 0, f"{env}:\n" + r.stdout[-6000:] + r.stderr[-3000:]
    seen = []
    for line in r.stdout.splitlines():
        if line.startswith("LAYERS-FORM "):
            seen.append(json.loads(line[len("LAYERS-FORM "):]))
            print(line)
    assert seen, r.stdout[-3000:]
    return seen


@pytest.mark.parametrize("variant,env", VARIANTS)
def test_edge_nets_under_kernel_variant(variant, env):
    """E1, E5, E6 and E13 in bf16x3 under a kernel variant, in a child process (the variables are read once per process)."""
    seen = _child(env, 240)
    forms = {f for _, f, _, _, _ in seen}
    if "BSMI_WINO4" in env:
        assert "winograd F(4x4)" in forms and "gather" not in forms, forms
    if "BSMI_H16" in env:
        assert "halo-resident" in forms, forms


# ---- every class was reached -----------------------------------------------------------------------------------------------------
# (BN, N-tiles, exact fit, form, flags the launch must carry) per precision, by hand from the table of tests/edge_nets.py.  split-k
# is left out of the required flags: the launcher sets it from the tile count and the card's CUs, not from the channel counts.
_G, _W, _RH = "gather", "winograd F(4x4)", "raster-halo"
_DIRECT = [
    (32, 1, False, _G, ()),        # 16 of 32 columns (E1), 11, 13, 23
    (32, 1, True, _G, ()),         # E4, E11: level 0 at 32
    (64, 1, True, _G, ()),         # E1: 64 exact; E6, E9 level 0
    (64, 1, False, _G, ()),        # E2: 33, one over the 32-column tile
    (160, 1, False, _G, ()),       # E3: 65, one over 64
    (160, 1, True, _G, ()),        # E4: 160 exact
    (256, 1, False, _G, ()),       # E5: 161, a single 256-column tile with 95 padding columns
    (256, 1, True, _G, ()),        # E6
    (320, 1, False, _G, ()),       # E7 (304), E8 (305)
    (320, 1, True, _G, ()),        # E9
    (256, 2, False, _G, ()),       # E10 (400), E11 (480)
    (320, 2, False, _G, ()),       # E12 (528)
    (320, 2, True, _G, ()),        # E13 (640)
    (64, 1, True, _RH, ()),        # E6, E9: the decoder's first stage of 64 columns
]
EXPECTED = {
    "f32": _DIRECT,
    "bf16": _DIRECT + [(0, 0, False, "first-pass", ()), (0, 0, False, "box-halo", ())],     # E1, E7, E12: level 0 at 16
    "bf16x3": [
        (0, 0, False, "first-pass", ()),             # E1, E7, E12
        (32, 1, False, _G, ()), (32, 1, True, _G, ()), (64, 1, True, _G, ()), (64, 1, False, _G, ()), (160, 1, False, _G, ()),
        (160, 1, True, _W, ()),                      # E4: F(4x4) at Cpad 160
        (256, 1, False, _G, ()), (256, 1, False, _W, ()),   # E5: both stages of 161 columns; Cpad 176 in the Winograd V
        (256, 1, True, _W, ()),                      # E6
        (320, 1, False, _G, ()),                     # E7: 16 -> 304, the fused 320-column tile with CUT
        (320, 1, False, _W, ()),                     # E7, E8
        (320, 1, True, _W, ()),                      # E9
        (256, 2, False, _G, ()), (256, 2, False, _W, ()),   # E10, E11
        (320, 2, False, _G, ()), (320, 2, False, _W, ()),   # E12
        (320, 2, True, _W, ()),                      # E13
        (64, 1, True, _W, ("fused-up",)),            # E6, E9: 320 / 384 -> 64, convolved below the upsampling
        (64, 1, True, _W, ("fused-up", "res-low")),  # ... and the narrow last stage
        (64, 1, False, _W, ("fused-up",)),           # E8 (61), E10 (40)
        (32, 1, True, _W, ("fused-up",)),            # E11: 512 -> 32, the rule's cout >= 32 edge
        (160, 1, True, _W, ("fused-up",)),           # E13: 800 -> 160
    ],
}
# output channel counts that a (BN, N-tiles) class must have met, where the table names two sides of a boundary
EXPECTED_COUTS = {(320, 1): {304, 305, 320}, (256, 2): {400, 480}, (64, 1): {33, 64}, (160, 1): {65, 160}, (256, 1): {161, 256}}
# stages that convolve below the upsampling, by output channels: dense at Cpad 64 (64, 61), 48 (40), 32 (32); batched at 160
EXPECTED_BELOW_UP = {64, 61, 40, 32, 160}


def test_every_tile_and_padding_class_was_reached():
    """The launches of the default rule over case E, as Model.plan_steps() reports them, contain every class the nets exist for.
    (last in the module: it needs test_case_e_edge_nets to have run)"""
    if _STOP:
        pytest.skip(f"a child process died earlier ({_STOP[0]})")
    for line in RECORD.lines():
        print(line)
    for prec in T.PRECS:
        for k, tag in sorted(CLASSES.get(prec, {}).items()):
            print(f"EDGE-CLASS {prec:7s} BN {k[0]:3d} x {k[1]} {'exact' if k[2] else '     '} {k[3]:16s} {' '.join(k[4]):20s} first in {tag}")
    print("EDGE-COUTS", {k: sorted(v) for k, v in sorted(COUTS.items())})
    print("EDGE-BELOW-UP", sorted(BELOW_UP))
    print("EDGE-HEAD largest err / bound per input channel count", HEAD_WORST)
    for prec, want in EXPECTED.items():
        have = CLASSES.get(prec, {})
        missing = [k for k in want if not any(h[:4] == k[:4] and set(k[4]) <= set(h[4]) for h in have)]
        assert not missing, f"{prec}: no net of case E reached {missing}"
        for (bn, nt), couts in EXPECTED_COUTS.items():
            assert couts <= COUTS.get((prec, bn, nt), set()), (prec, bn, nt, sorted(COUTS.get((prec, bn, nt), set())))
    assert EXPECTED_BELOW_UP <= {c for p, c in BELOW_UP if p == "bf16x3"}, sorted(BELOW_UP)


# ---- child process ------------------------------------------------------------------------------------------------------------
def _main(what):
    assert what == "variant", what
    rec = T.Record()
    for tag in E.VARIANT_TAGS:
        run_edge(tag, "bf16x3", rec)
    print("\n".join(rec.lines()))


if __name__ == "__main__":
    _main(sys.argv[1])
