"""Per-launch parity of the U-Net forward: after one forward, EVERY step of the plan is read back (Model.debug_activation)
and its output compared with a float64 computation of that one operation on the step's own inputs as the device holds
them (tests/layer_ref.py).  Needs an MI355X.

  input  f32: bit-equal to oracle.unet_ref.normalize_raw / normalize_unit (the kernel's x * 2 + -1 may contract to an fma: x * 2
         is exact, so the bits are the same); other modes within the storage rounding g_out
  pool   bit-equal to the max over the device's own input, every mode
  up     |got - ref| <= (g_out + 9 * 2^-24) * upsample(|x|): the weights 1/4, 3/4 are exact, the kernel interpolates in f32 --
         three linear interpolations of two products and a sum each -- and stores once.  A factor that is no power of two (the
         factor-3 net of case B) has weights that f32 does not hold: their rounding is allowed for as derived in
         layer_ref.Upsampled.weight_error (found by this suite's first run: 592 elements of that map were off by up to 6e-7)
  conv   |got - ref| <= g_acc * S + g_out * |ref| element-wise, g_acc = 4 * max(e_fmt, e_acc32) from the reference alone
         (layer_ref); the first ConvPass as one launch (first_pass) is checked as the chain of its two stages from the raw input
  head   |got - ref| <= G_HEAD, the f32 outputs of the forward against float64 from the device's last trunk activation
  and the plan walker agrees with Model.plan_steps() (types, shapes, prefixes), non-materialised steps raise.

Gates.  g_out = 2^-24 (f32), 2^-17 (split), 2^-8 (bf16: 8 significant bits, round to nearest even; layer_ref) are derived.  g_acc is computed per step from
the emulation of the step's form and the f32 accumulation allowance, on a seeded sample of at most 2048 of the step's own rows
(a sample can only make the gate tighter); case D too computes both per step -- the Winograd emulation on a block of the step
that holds its last two tile rows; the sequential f32 sum always runs on 512 of the sampled rows and at most 64 channels.  G_HEAD is the one MEASURED gate: the largest error of
the head kernel (f32 fma chains over at most 12 channels, expf, 1 / (1 + e)) against float64 over cases A-C on the MI355X,
times 4.

Largest err / S seen per (precision, form) on the MI355X with the gate it was held against (records, not gates; the tests
print them as `LAYERS-FORM` lines):

  precision  form               largest err / S   largest g_acc of those steps
  f32        gather             3.78e-05          3.95e-05   (full net, r_conv.0.2 conv 0, K = 48 600, split-K; the others <= 2.0e-05)
  f32        raster-halo        1.47e-05          4.78e-05
  bf16x3     gather             5.06e-05          8.29e-05
  bf16x3     first-pass         3.35e-05          9.56e-05
  bf16x3     halo-resident      3.20e-05          8.01e-05
  bf16x3     winograd F(2x2)    4.16e-05          1.39e-04
  bf16x3     winograd F(4x4)    1.69e-04          5.96e-04
  bf16       gather             1.63e-02          3.02e-02
  bf16       raster-halo        1.45e-02          3.02e-02
  bf16       box-halo           1.18e-02          2.24e-02
  bf16       first-pass         1.85e-02          4.39e-02
  head (every mode)             1.68e-07 absolute, gate 6.73e-07
(err / S contains the rounding of the stored output, g_out |ref| / S, which the gate allows on top of g_acc S: where |ref| >> S
it can exceed the step's g_acc.  No step of any case or variant exceeded its gate; the suite's findings were on the reference's
side: the f32 interpolation weights of a factor-3 upsampling, and the f32 MFMA rounding its accumulator every 2 products.)
Wall time on the MI355X with all variant children: 14 min 46 s; tests/test_layers_cpu.py: 14 s on 8 threads.

Cases: A the golden and family nets, every element, three precisions; B the random ragged nets, every element, f32 and
bf16x3; C 12 / 60 / 300 channels at (22, 116, 116) and at a ragged shape whose last M-tiles and last F(4x4) tiles are partial,
every element, three precisions; D the full net at (156, 220, 220), conv steps sampled (layer_ref.sample_voxels), the rest in
full.  The kernel variants of tests/test_fullsize_gpu.py CONV_KERNEL_VARIANTS run a thinned set of A-C in a child process
each, the variants that change what a full-size layer runs also case D.
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

import layer_ref as L  # noqa: E402

pytestmark = pytest.mark.gpu

PRECS = ["f32", "bf16x3", "bf16"]
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
# measured against float64 on the MI355X over cases A-C (largest |got - ref| of any head output: HEAD_MEASURED), margin 4
HEAD_MEASURED = 1.682e-7
G_HEAD = 4 * HEAD_MEASURED
G_UP_ARITH = 9 * 2.0 ** -24
GATE_SAMPLE = 2048      # rows on which a step's allowances are computed
ACC_SAMPLE = 512        # ... and its sequential f32 sum in case D

ALL_FORMS = ("gather", "raster-halo", "box-halo", "halo-resident", "first-pass", "winograd F(2x2)", "winograd F(4x4)")
ALL_FLAGS = ("fused-up", "res-low", "split-k")


# ---- nets ---------------------------------------------------------------------------------------------------------------
GOLDEN = ["affs_f4i2", "affs_f3i3", "mtlsd_f4i2"]
FAMILY = ["2d_mtlsd_f4i2", "2d_lsd_f3i3", "2d_affs_f4i2", "3d_lsd_f4i2", "from_2d_mtlsd_f3i2", "from_3d_lsd_f4i2", "from_2d_affs_f4i3"]
C_NET = {"in_channels": 1, "num_fmaps": 12, "fmap_inc_factor": 5, "downsample_factors": [[1, 2, 2], [1, 2, 2]],
         "kernel_size_down": [[[3, 3, 3], [3, 3, 3]]] * 3, "kernel_size_up": [[[3, 3, 3], [3, 3, 3]]] * 2, "outputs": {"3d_affs": {"dims": 6}}}
# (22, 116, 116) and a ragged one, W != H: the stage outputs are (.., 110, 122), (.., 47, 53), (.., 19, 22), (.., 30, 36), ... --
# no multiples of 4 among the 300- and 60-channel stages (overhanging F(4x4) tiles) and row counts that are no multiples of 256
C_SHAPES = [(22, 116, 116), (21, 120, 132)]
D_SHAPE = (156, 220, 220)


def golden_case(tag):
    from test_unet_gpu import _load, _net_config
    d, sd, meta = _load(GOLDEN_DIR, tag)
    return _net_config(meta), sd, d["raw_u8"]


def family_net(tag):
    from test_oracle_unet import family_case
    nc, sd, ins, _, _ = family_case(GOLDEN_DIR, tag)
    raw = np.concatenate(ins, axis=0) if len(ins) > 1 else ins[0]
    if len(nc["downsample_factors"][0]) == 2:
        raw = raw[:, None]
    return nc, sd, raw


def ragged_case(i):
    from test_unet_gpu import random_ragged_nets
    c, cfg, sd, raw = list(random_ragged_nets())[i]
    return dict(cfg, outputs={"3d_affs": {"dims": 6}}), sd, raw


def c_case(shape):
    from bootstrapper_amd.synth import synthetic_state_dict
    raw = np.random.default_rng(7).integers(0, 256, size=shape, dtype=np.uint8)
    return C_NET, synthetic_state_dict(C_NET, 3), raw


def d_case():
    from bootstrapper_amd.synth import synthetic_state_dict, synthetic_volume
    from test_lib_cpu import AFFS_NET_CONFIG
    return AFFS_NET_CONFIG, synthetic_state_dict(AFFS_NET_CONFIG, 0), synthetic_volume(D_SHAPE, 3, device="cpu").numpy()


# ---- one case -----------------------------------------------------------------------------------------------------------
class Record:
    """largest err / S and the gate it met, per (precision, form, flags)"""

    def __init__(self):
        self.forms = {}
        self.head = 0.0

    def add(self, prec, form, flags, es, g_acc):
        k = (prec, form, flags)
        old = self.forms.get(k, (0.0, 0.0))
        self.forms[k] = (max(old[0], es), max(old[1], g_acc))

    def lines(self):
        out = [f"LAYERS-FORM {json.dumps([p, f, list(fl), es, g])}" for (p, f, fl), (es, g) in sorted(self.forms.items())]
        return out + [f"LAYERS-HEAD {self.head:.4e}"]


RECORD = Record()


def _w5(a):
    a = np.asarray(a, dtype=np.float32)
    return a[:, :, None] if a.ndim == 4 else a


def _chunks(n, k):
    rows = max(512, int(4e7 // max(k, 1)))
    return [(a, min(a + rows, n)) for a in range(0, n, rows)]


def _conv3d_f64(x, w, b):
    """(D, H, W, C) float64, OIDHW float64 -> valid conv (D', H', W', O) by torch"""
    t = torch.from_numpy(np.ascontiguousarray(x.transpose(3, 0, 1, 2)))[None]
    with torch.no_grad():
        y = torch.nn.functional.conv3d(t, torch.from_numpy(np.ascontiguousarray(w)), torch.from_numpy(b))
    return y[0].numpy().transpose(1, 2, 3, 0)


def _block_input(src, zr, yr, xr):
    """The (cropped, concatenated) input of a stage on a block of its input voxels, float32 as the device holds it (an upsampled
    map that was never written: the reference upsampling, rounded to f32)."""
    z, y, x = np.meshgrid(np.arange(*zr), np.arange(*yr), np.arange(*xr), indexing="ij")
    parts = [t.at(z.ravel() + org[0], y.ravel() + org[1], x.ravel() + org[2]) for t, org, _ in src]
    return np.concatenate(parts, axis=1).astype(np.float32).reshape(z.shape + (-1,))


def run_case(case, nc, sd, raw, prec, sampled=False, record=RECORD):
    """One forward of the net on `raw` (u8, (D, H, W) or (C, D, H, W)) in `prec`, then every step against its reference."""
    from bootstrapper_amd.unet import Model
    from bootstrapper_amd._lib import BsmiError, ERR_STATE
    from oracle import unet_ref as R
    t_start = time.time()
    m = Model(nc, precision=prec).load_state_dict(sd)
    u8, f32 = m.predict_u8(torch.from_numpy(np.ascontiguousarray(raw)).cuda(), want_f32=True)
    torch.cuda.synchronize()
    heads_out = [t.cpu().numpy() for t in f32]
    plan = m.plan_steps()
    shape = tuple(raw.shape[-3:])
    ops = L.walk(nc, shape)
    L.check_walk(ops, plan)
    g_out = L.G_OUT[prec]
    rng = np.random.default_rng(12345)
    x_norm = (R.normalize_raw(raw) if "in_channels" in nc else R.normalize_unit(raw))
    x_norm = (x_norm[None] if x_norm.ndim == 3 else x_norm).transpose(1, 2, 3, 0)      # (D, H, W, C) float32

    # how long a step's tensor is needed: its last reader; a step that is not materialised hands the need on to its source
    last_use = {}
    for i, o in enumerate(ops):
        srcs = [s for s, _, _ in o.get("src", [])] + [s for s, _, _ in (o.get("res") or [])] if o["type"] == "conv" else ([o["src"]] if "src" in o else [])
        for s in srcs:
            last_use[s] = max(last_use.get(s, -1), i)
    for i in range(len(ops) - 1, -1, -1):
        if not plan[i]["materialised"] and ops[i]["type"] == "up":
            last_use[ops[i]["src"]] = max(last_use.get(ops[i]["src"], -1), last_use.get(i, -1))
    held = {}

    def tensor(step):
        if plan[step]["materialised"]:
            return held[step]
        o = ops[step]
        assert o["type"] == "up", (step, o["type"])
        return L.Upsampled(held[o["src"]], o["factor"], o["offset"], o["shape"])

    def where(i):
        p = plan[i]
        extra = f" {p['prefix']} conv {p['conv']} [{p['form']}{''.join(' ' + f for f in p['flags'])}, BN {p['bn']}, {p['ksteps']} K-steps]" if p["type"] == "conv" else ""
        return f"{case} {prec} step {i} ({p['type']}{extra}, shape {p['shape']})"

    for i, (o, p) in enumerate(zip(ops, plan)):
        if not p["materialised"]:
            with pytest.raises(BsmiError) as ei:
                m.debug_activation(i)
            assert ei.value.code == ERR_STATE and "not materialised" in ei.value.msg, where(i)
            continue
        if o["type"] == "head":
            z = held[o["src"]].a.astype(np.float64).reshape(-1, held[o["src"]].shape[3])
            w1, b1 = _w5(sd[o["prefix"] + ".conv_pass.0.weight"])[:, :, 0, 0, 0].astype(np.float64), sd[o["prefix"] + ".conv_pass.0.bias"].astype(np.float64)
            w2, b2 = _w5(sd[o["prefix"] + ".residual.0.weight"])[:, :, 0, 0, 0].astype(np.float64), sd[o["prefix"] + ".residual.0.bias"].astype(np.float64)
            y = (z @ w1.T + b1) + (z @ w2.T + b2)
            ref = 1.0 / (1.0 + np.exp(-y))
            got = heads_out[p["head"]].reshape(ref.shape[1], -1).T.astype(np.float64)
            err = np.abs(got - ref)
            record.head = max(record.head, float(err.max()))
            print(f"{where(i)}: head max abs err {err.max():.3e} (gate {G_HEAD:.3e})")
            assert err.max() <= G_HEAD, f"{where(i)}: head err {err.max():.3e} > {G_HEAD:.3e} at row {int(err.max(axis=1).argmax())}"
            continue
        got = m.debug_activation(i)
        assert got.shape == tuple(o["shape"]), where(i)
        assert np.isfinite(got).all(), where(i)
        if o["type"] == "input":
            if prec == "f32":
                assert np.array_equal(got, x_norm), where(i)
            else:
                assert np.all(np.abs(got.astype(np.float64) - x_norm) <= g_out * np.abs(x_norm)), where(i)
        elif o["type"] == "pool":
            assert np.array_equal(got, L.maxpool(held[o["src"]].a, o["factor"])), where(i)
        elif o["type"] == "up":
            up = L.Upsampled(held[o["src"]], o["factor"], o["offset"], o["shape"])
            bad = np.abs(got - up.full()) > (g_out + G_UP_ARITH) * up.full(np.abs) + up.weight_error() * up.full(np.abs, unit_weights=True)
            assert not bad.any(), f"{where(i)}: {int(bad.sum())} elements off, first at {tuple(int(v[0]) for v in np.nonzero(bad))}"
        else:
            _check_conv(case, prec, i, o, p, got, sd, tensor, x_norm, sampled, rng, record, where, plan)
        held[i] = L.Dense(got)
        for s in [s for s in held if last_use.get(s, -1) <= i]:
            del held[s]
    del m
    print(f"{case} {prec}: {len(ops)} steps checked in {time.time() - t_start:.1f} s")


def _check_conv(case, prec, i, o, p, got, sd, tensor, x_norm, sampled, rng, record, where, plan):
    g_out = L.G_OUT[prec]
    shape = tuple(o["shape"])
    pre_key = f"{o['prefix']}.conv_pass.{2 * o['conv']}"
    form, flags = p["form"], tuple(p["flags"])
    wino_m = {"winograd F(2x2)": 2, "winograd F(4x4)": 4}.get(form, 0)
    first = form == "first-pass"
    if first:
        # the whole first ConvPass from the raw input: stage 0 in float64 (and as the mode computes and stores it), then stage 1
        assert o["conv"] == 1 and not plan[i - 1]["materialised"], where(i)
        x = L.Dense(L.store(x_norm, prec))
        k0 = f"{o['prefix']}.conv_pass.0"
        w0, b0 = _w5(sd[k0 + ".weight"]), np.asarray(sd[k0 + ".bias"], np.float32)
        x64 = x.full()
        a1 = np.maximum(_conv3d_f64(x64, w0.astype(np.float64), b0.astype(np.float64)), 0.0)
        if prec == "bf16":
            e1 = _conv3d_f64(x64, L.bf16_rne(w0).astype(np.float64), b0.astype(np.float64))
        else:
            wh, wl = L.split_bf16(w0)
            e1 = _conv3d_f64(x64, wh, b0.astype(np.float64)) + _conv3d_f64(L.bf16_rne(x.a).astype(np.float64), wl, np.zeros(len(b0)))
        a1_emu = L.Dense(L.store(np.maximum(e1, 0.0), prec))
        src = [(L.Dense(a1), (0, 0, 0), a1.shape[3])]
        res = [(x, (2, 2, 2), x.shape[3])]
    else:
        src = [(tensor(s), org, c) for s, org, c in o["src"]]
        res = [(tensor(s), org, c) for s, org, c in o["res"]] if o["res"] else None
    wr = _w5(sd[o["prefix"] + ".residual.0.weight"]) if res else None
    br = sd[o["prefix"] + ".residual.0.bias"] if res else None
    st = L.Stage(src, o["kernel"], _w5(sd[pre_key + ".weight"]), sd[pre_key + ".bias"], res, wr, br)
    K = st.W.shape[0]

    # -- the gate, from the reference alone, on a sample of the step's rows
    M = shape[0] * shape[1] * shape[2]
    if sampled:
        vox = L.sample_voxels(shape, 2048, rng, wino_m)
    else:
        vox = L.all_voxels(shape)
    if M <= GATE_SAMPLE:
        gsel = np.arange(len(vox[0]))
    else:
        gsel = np.unique(np.concatenate([[0, len(vox[0]) - 1], rng.integers(0, len(vox[0]), size=GATE_SAMPLE)]))
    gv = tuple(v[gsel] for v in vox)
    Xg = st.rows(*gv)
    pre_g, S_g = st.ref(Xg)
    emu = f32_pre = None
    if first:
        st_e = L.Stage([(a1_emu, (0, 0, 0), a1_emu.shape[3])], o["kernel"], _w5(sd[pre_key + ".weight"]), sd[pre_key + ".bias"], res, wr, br)
        emu = st_e.emulate(st_e.rows(*gv), prec)
    elif wino_m and not sampled:
        full = L.wino_emulate(_block_input(src, (0, shape[0] + 2), (0, shape[1] + 2), (0, shape[2] + 2)), _w5(sd[pre_key + ".weight"]), wino_m)
        emu = full[gv] + st.bias + (st.emulate(Xg, prec, part="res") if res else 0.0)
    elif wino_m:
        # case D: the transform's arithmetic on a block of the step -- two planes, the last two tile rows (the overhanging one
        # among them), the full width -- in place of the sampled rows
        z0, y0 = shape[0] // 2, max(0, (-(-shape[1] // wino_m) - 2) * wino_m)
        blk = L.wino_emulate(_block_input(src, (z0, z0 + 4), (y0, shape[1] + 2), (0, shape[2] + 2)), _w5(sd[pre_key + ".weight"]), wino_m)
        bz, by, bx = np.meshgrid(np.arange(2), np.arange(shape[1] - y0), np.arange(shape[2]), indexing="ij")
        gv = (bz.ravel() + z0, by.ravel() + y0, bx.ravel())
        Xg = st.rows(*gv)
        pre_g, S_g = st.ref(Xg)
        emu = blk.reshape(-1, blk.shape[3]) + st.bias + (st.emulate(Xg, prec, part="res") if res else 0.0)
        gsel = np.zeros(0)   # (these rows are not the compared ones)
    if not sampled:
        f32_pre = L.conv3d_f32(st, shape)[gv]
    if sampled and len(Xg) > ACC_SAMPLE:
        # case D: the format error on GATE_SAMPLE rows, the accumulation allowance (as many small GEMMs as the stage has K-steps) on
        # ACC_SAMPLE of them
        e_fmt = L.norm_err(st.emulate(Xg, prec) if emu is None else emu, pre_g, S_g)
        asel = rng.choice(len(Xg), ACC_SAMPLE, replace=False)
        _, e_acc = L.allowances(st, Xg[asel], pre_g[asel], S_g[asel], prec, bool(wino_m), "split-k" in flags, emu_pre=pre_g[asel])
    else:
        e_fmt, e_acc = L.allowances(st, Xg, pre_g, S_g, prec, bool(wino_m), "split-k" in flags, emu_pre=emu, f32_pre=f32_pre)
    g_acc = L.gate(e_fmt, e_acc)

    # -- every (sampled) element
    worst_es = 0.0
    n = len(vox[0])
    for a, b in _chunks(n, K):
        cv = tuple(v[a:b] for v in vox)
        if a == 0 and b == n and len(gsel) == n:
            pre, S = pre_g, S_g
        else:
            pre, S = st.ref(st.rows(*cv))
        ok, worst = L.compare(got[cv].astype(np.float64), st.act(pre), S, g_acc, g_out)
        worst_es = max(worst_es, worst["max_err_over_S"])
        assert ok, (f"{where(i)}: {L.describe(worst, cv, shape)}; g_acc {g_acc:.3e} = 4 * max(e_fmt {e_fmt:.3e}, e_acc32 {e_acc:.3e}), "
                    f"g_out {g_out:.3e}")
    record.add(prec, form, flags, worst_es, g_acc)
    print(f"{where(i)}: K {K}, {n} voxels, max err/S {worst_es:.3e}, g_acc {g_acc:.3e} (e_fmt {e_fmt:.3e}, e_acc32 {e_acc:.3e})")


# ---- the default rule, in this process --------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tag", GOLDEN + FAMILY)
def test_case_a_golden_and_family_nets(tag, prec):
    nc, sd, raw = golden_case(tag) if tag in GOLDEN else family_net(tag)
    run_case(f"A:{tag}", nc, sd, raw, prec)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("idx", [0, 1, 2])
def test_case_b_random_ragged_nets(idx, prec):
    nc, sd, raw = ragged_case(idx)
    run_case(f"B:{idx}", nc, sd, raw, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", C_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_case_c_12_60_300_channels(shape, prec):
    nc, sd, raw = c_case(shape)
    run_case(f"C:{shape}", nc, sd, raw, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_case_d_full_net_sampled(prec):
    nc, sd, raw = d_case()
    run_case("D", nc, sd, raw, prec, sampled=True)


# ---- the kernel variants, a child process each ---------------------------------------------------------------------------------
def _variants():
    from test_fullsize_gpu import CONV_KERNEL_VARIANTS
    return CONV_KERNEL_VARIANTS


# case D again in bf16x3 under the variants that change what a full-size layer runs
D_VARIANTS = [
    ("no Winograd stage", {"BSMI_WINO": "0"}),
    ("F(4x4) on every stage", {"BSMI_WINO": "2", "BSMI_WINO4": "2"}),
    ("no F(4x4) stage", {"BSMI_WINO4": "0"}),
    ("no halo-resident stage", {"BSMI_H16": "0"}),
    ("halo-resident form on every narrow stage", {"BSMI_H16": "2"}),
    ("upsampled maps materialised", {"BSMI_FUSE_UP": "0"}),
    ("no first_pass / conv_box", {"BSMI_FUSED_FIRST": "0", "BSMI_USE_BOX": "0"}),
    ("forced split-K", {"BSMI_SK_GRID": "8", "BSMI_TILE_EFF": "0.01,0.01,0.01,1,0.01"}),
]

_SEEN = {}            # (form or flag) -> variant that met it, over the whole module run
_STOP = []            # a child ended on a signal or a timeout: no further GPU work in this run
_DEAD = (134, 139, 124, 137, -6, -11, -9)


def _child(what, env, timeout):
    if _STOP:
        pytest.skip(f"a child process died earlier ({_STOP[0]}): no further GPU work in this run")
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), what], env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=timeout, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _STOP.append(f"{what} {env}: timeout after {timeout} s")
        raise
    if r.returncode in _DEAD:
        _STOP.append(f"{what} {env}: exit status {r.returncode}")
    assert r.returncode == 0, f"{env}:\n" + r.stdout[-6000:] + r.stderr[-3000:]
    seen = []
    for line in r.stdout.splitlines():
        if line.startswith("LAYERS-FORM "):
            prec, form, flags, es, g = json.loads(line[len("LAYERS-FORM "):])
            seen.append((prec, form, tuple(flags), es, g))
            for k in [form] + flags:
                _SEEN.setdefault(k, str(env))
            print(line)
    assert seen, r.stdout[-3000:]
    return seen


@pytest.mark.parametrize("variant,env", _variants())
def test_thinned_cases_under_kernel_variant(variant, env):
    """Case C at both shapes, one golden, one family and one ragged net under a kernel variant, in a child process (the variables
    are read once per process)."""
    _child("thin-split" if set(env) <= _SPLIT_ONLY else "thin", env, 300)


@pytest.mark.parametrize("variant,env", D_VARIANTS)
def test_case_d_under_kernel_variant(variant, env):
    _child("D", env, 600)


def test_every_form_and_flag_was_reached():
    """The union over this module's run -- the default rule in this process, the variant children -- covers every kernel form and
    every flag bsmi_unet_debug_step_info can report.  (last in the module: it needs the tests above to have run)"""
    if _STOP:
        pytest.skip(f"a child process died earlier ({_STOP[0]})")
    seen = dict(_SEEN)
    for (prec, form, flags) in RECORD.forms:
        for k in (form,) + tuple(flags):
            seen.setdefault(k, "default rule")
    print({k: seen.get(k) for k in ALL_FORMS + ALL_FLAGS})
    for (prec, form, flags), (es, g) in sorted(RECORD.forms.items()):
        print(f"default rule: {prec:7s} {form:16s} {' '.join(flags):24s} max err/S {es:.3e}  gate {g:.3e}")
    missing = [k for k in ALL_FORMS + ALL_FLAGS if k not in seen]
    assert not missing, f"no case reached {missing}"


# ---- child process ----------------------------------------------------------------------------------------------------------
# variables that only the split-bf16 mode reads: a variant made of these alone runs its thinned cases in that mode only
_SPLIT_ONLY = {"BSMI_WINO", "BSMI_WINO4", "BSMI_FUSE_UP", "BSMI_H16", "BSMI_X3_FUSED", "BSMI_WINO_PACK_HOST"}


def _main(what):
    rec = RECORD
    if what.startswith("thin"):
        for prec in (["bf16x3"] if what == "thin-split" else PRECS):
            for shape in C_SHAPES:
                run_case(f"C:{shape}", *c_case(shape), prec)
            run_case("A:affs_f4i2", *golden_case("affs_f4i2"), prec)
            run_case("A:from_2d_mtlsd_f3i2", *family_net("from_2d_mtlsd_f3i2"), prec)
            if prec != "bf16":
                run_case("B:1", *ragged_case(1), prec)
    elif what == "D":
        run_case("D", *d_case(), "bf16x3", sampled=True)
    else:
        raise SystemExit(f"unknown child job {what!r}")
    print("\n".join(rec.lines()))


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    _main(sys.argv[1])
