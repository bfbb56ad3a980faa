"""The per-launch comparison of tests/layer_ref.py has to detect: on synthetic stages, with emulations of the kernels'
arithmetic standing in for the kernels, every emulation passes the gate that tests/test_layers_gpu.py holds the MI355X
to, and every injected fault fails it.  No GPU.  The stages e64 / e65 / e161 / e305 stand at the channel counts of case E
(tests/edge_nets.py) with the faults of a tile or padding edge: EDGE_FAULT_CASES.

Gates as in layer_ref: |got - ref| <= g_acc S + g_out |ref| with g_acc = 4 max(e_fmt, e_acc32), both from the reference.
"""
import os

import numpy as np
import pytest
import torch

import layer_ref as L

torch.set_num_threads(min(16, os.cpu_count() or 1))

PRECS = ["f32", "bf16x3", "bf16"]


def _weights(rng, cout, cin, k, gain=1.5):
    fan = cin * k[0] * k[1] * k[2]
    return ((rng.standard_normal((cout, cin, *k)) * (gain / np.sqrt(fan))).astype(np.float32),
            (rng.standard_normal(cout) * 0.1).astype(np.float32))


def _acts(rng, shape, prec):
    """post-ReLU activations as the mode stores them"""
    return L.store(np.maximum(rng.standard_normal(shape), 0), prec)


def make_stage(name, prec, seed=0):
    """(stage, output shape).  Stages: 3x3x3 with Cin / Cout = 12/12, 60/60, 300/64; one (1,3,3) stage; `rconv`: the single stage
    of an r_conv pass over the concatenation of a cropped skip connection and an upsampled map, with its residual branch."""
    rng = np.random.default_rng(seed)
    if name == "rconv":
        k = (3, 3, 3)
        low = L.Dense(_acts(rng, (5, 9, 8, 40), prec))
        up = L.Upsampled(low, (1, 2, 2), (0, 1, 1), (5, 16, 14, 40))
        if prec == "f32":   # a materialised map holds stored values
            up = L.Dense(L.store(up.full(), prec))
        skip = L.Dense(_acts(rng, (7, 20, 19, 24), prec))
        so = (1, 2, 2)
        w, b = _weights(rng, 24, 64, k)
        wr, br = _weights(rng, 24, 64, (1, 1, 1), gain=1.0)
        src = [(skip, so, 24), (up, (0, 0, 0), 40)]
        res = [(skip, tuple(o + 1 for o in so), 24), (up, (1, 1, 1), 40)]
        return L.Stage(src, k, w, b, res, wr, br), (3, 14, 12, 24)
    cin, cout, k, shape = {"c12": (12, 12, (3, 3, 3), (6, 14, 15)), "c60": (60, 60, (3, 3, 3), (5, 16, 15)),
                           "c300": (300, 64, (3, 3, 3), (5, 16, 15)), "k133": (60, 60, (1, 3, 3), (3, 16, 15)),
                           # the channel counts of tests/edge_nets.py: an exact fit of the 64-column tile, one over it, one over 160
                           # (eleven 16-channel units), and 304 of 320 columns read from twenty units, the last with one channel
                           "e64": (64, 64, (3, 3, 3), (5, 12, 13)), "e65": (65, 65, (3, 3, 3), (5, 12, 13)),
                           "e161": (161, 161, (3, 3, 3), (5, 12, 13)), "e305": (305, 304, (3, 3, 3), (5, 12, 13))}[name]
    x = L.Dense(_acts(rng, shape + (cin,), prec))
    w, b = _weights(rng, cout, cin, k)
    return L.Stage([(x, (0, 0, 0), cin)], k, w, b), tuple(shape[d] - k[d] + 1 for d in range(3)) + (cout,)


STAGES = ["c12", "c60", "c300", "k133", "rconv"]


def _setup(name, prec):
    st, shape = make_stage(name, prec)
    vox = L.all_voxels(shape)
    X = st.rows(*vox)
    pre, S = st.ref(X)
    e_fmt, e_acc = L.allowances(st, X, pre, S, prec)
    return st, shape, vox, X, pre, S, L.gate(e_fmt, e_acc), e_fmt, e_acc


def _check(st, got_pre, pre, S, g_acc, prec, relu=True):
    got = L.store(st.act(got_pre) if relu else got_pre, prec).astype(np.float64)
    return L.compare(got, st.act(pre), S, g_acc, L.G_OUT[prec])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", STAGES)
def test_emulation_passes_its_own_gate(name, prec):
    st, shape, vox, X, pre, S, g_acc, e_fmt, e_acc = _setup(name, prec)
    print(f"{name} {prec}: K = {X.shape[1]}  e_fmt {e_fmt:.3e}  e_acc32 {e_acc:.3e}  g_acc {g_acc:.3e}")
    ok, worst = _check(st, st.emulate(X, prec), pre, S, g_acc, prec)
    assert ok, L.describe(worst, vox, shape)
    # ... and so does f32 accumulation of the same products in the kernel's K order (also with a split-K cut) and in torch's
    if prec == "f32":
        ok, worst = _check(st, st.acc32_torch(X), pre, S, g_acc, prec)
        assert ok, L.describe(worst, vox, shape)
        for split_k in (False, True):
            acc, pre_s, S_s = st.acc32_sequential(X, prec, split_k=split_k, max_rows=1 << 30, max_cols=1 << 30)
            assert np.array_equal(pre_s, pre) or np.abs(pre_s - pre).max() < 1e-12
            ok, worst = _check(st, acc, pre, S, g_acc, prec)
            assert ok, L.describe(worst, vox, shape)


def test_format_errors_against_S_do_not_depend_on_K():
    """What makes one gate serve every layer (tools/layer_error_scales.py): split 1.9e-5 ... 2.2e-5 there."""
    e = {}
    for name in ("c12", "c60", "c300"):
        for prec in ("bf16x3", "bf16"):
            e[name, prec] = _setup(name, prec)[7]
    print(e)
    for prec, lo, hi in (("bf16x3", 8e-6, 4e-5), ("bf16", 4e-3, 2e-2)):
        v = [e[n, prec] for n in ("c12", "c60", "c300")]
        assert lo < min(v) and max(v) < hi and max(v) / min(v) < 2.5, (prec, v)


FAULTS = ["lo_tap", "kstep", "bias", "res_crop", "no_relu", "tile_shift"]


# The weights have a lo part in the split mode only; the residual branch exists on the r_conv stage only.  An omitted bias is
# asserted in f32 and in the split mode: the plain bf16 format cannot tell it from its own rounding (the pair is pinned by
# test_omitted_bias_is_inside_the_bf16_format below: err / S 1.3e-2 for the fault on the 60-channel stage, gate 2.9e-2).
FAULT_CASES = [(n, f, p) for n in STAGES for f in FAULTS for p in PRECS
               if not (f == "lo_tap" and p != "bf16x3") and not (f == "res_crop" and n != "rconv") and not (f == "bias" and p == "bf16")]


@pytest.mark.parametrize("name,fault,prec", FAULT_CASES)
def test_injected_fault_fails_the_gate(name, fault, prec):
    st, shape, vox, X, pre, S, g_acc, e_fmt, e_acc = _setup(name, prec)
    relu = True
    if fault == "lo_tap":
        bad = st.emulate(X, prec, fault=("lo_tap", len(st.taps) // 2))
    elif fault == "kstep":
        bad = st.emulate(X, prec, fault=("kstep", 1))
    elif fault == "bias":
        bad = st.emulate(X, prec, fault=("bias", 3))
    elif fault == "res_crop":
        bad = st.emulate(st.rows(*vox, res_shift=(0, 0, 1)), prec)
    elif fault == "no_relu":
        bad, relu = st.emulate(X, prec), False
    else:   # the rows of the second 256-row tile come from the voxel one further
        bad = st.emulate(X, prec)
        hi = min(2 * L.M_TILE, len(bad) - 1)
        bad[L.M_TILE:hi] = bad[L.M_TILE + 1:hi + 1]
    ok, worst = _check(st, bad, pre, S, g_acc, prec, relu)
    print(f"{name} {prec} {fault}: worst err/S {worst['max_err_over_S']:.3e} against g_acc {g_acc:.3e} (format {e_fmt:.3e})")
    assert not ok, f"{fault} passes the gate of {name} in {prec}: largest err/S {worst['max_err_over_S']:.3e}, g_acc {g_acc:.3e}"


def test_omitted_bias_is_inside_the_bf16_format():
    """The one (fault, gate) pair this comparison cannot separate: a bias of 0.1 sigma left out of one channel is 6e-3 ... 1.4e-1
    of S depending on the stage and the channel, and the bf16 format itself is 5.6e-3 ... 7.3e-3 of S, i.e. a gate of 2.2e-2 ...
    2.9e-2 with the margin of 4.  On the 60-channel stage the fault (1.3e-2) stays under the gate (2.9e-2); f32 (7e-6) and
    the split mode (5.8e-5) catch it everywhere.  A bf16 kernel that drops a bias is caught through its f32 / split twins, which
    share the epilogue, and by the end-to-end tests."""
    st, shape, vox, X, pre, S, g_acc, e_fmt, e_acc = _setup("c60", "bf16")
    ok, worst = _check(st, st.emulate(X, "bf16", fault=("bias", 3)), pre, S, g_acc, "bf16")
    print(f"omitted bias in bf16: err/S {worst['max_err_over_S']:.3e}, g_acc {g_acc:.3e}, format {e_fmt:.3e}")
    assert ok and e_fmt < worst["max_err_over_S"] < g_acc


# ---- the channel counts on the tile and padding edges (tests/edge_nets.py, tests/test_layers_edges_gpu.py) ------------------------
EDGE_STAGES = ["e64", "e65", "e161", "e305"]
# the column at which a second N-tile (or a second column half of a wide tile) of the stage begins
SECOND_TILE = {"e65": 64, "e161": 160, "e305": 256}
# exact_ulp     the last real column of a tile that the stage fills exactly has one product wrong by one bf16 ulp of its weight
# tile2_zero    the first column of a second N-tile zeroed
# unit_channel  one channel of the last 16-channel unit (the only real one where cin = 16 n + 1) left out of the sum, every tap
# pad_leak      a padding column's (zero) weights of one tap land in column cout - 1: that tap is missing there
# exact_ulp is asserted in f32 and in the split mode: one bf16 ulp of one product is what the bf16 mode's own weights carry on
# every product (pinned by test_one_bf16_ulp_of_one_product_is_inside_the_bf16_format)
EDGE_FAULT_CASES = ([("e64", "exact_ulp", p) for p in ("f32", "bf16x3")] +
                    [(n, "tile2_zero", p) for n in SECOND_TILE for p in PRECS] +
                    [(n, "unit_channel", p) for n in ("e65", "e161", "e305") for p in PRECS] +
                    [(n, "pad_leak", p) for n in ("e65", "e161", "e305") for p in PRECS])
_EDGE_SETUP = {}


def _edge_setup(name, prec):
    """_setup of an edge stage, computed once per (stage, precision) and shared; nothing changes it"""
    if (name, prec) not in _EDGE_SETUP:
        _EDGE_SETUP[name, prec] = _setup(name, prec)
    return _EDGE_SETUP[name, prec]


def _edge_fault(st, X, prec, fault, name):
    """the emulation's sums with one fault of EDGE_FAULT_CASES"""
    c = st.cols
    last = st.cout - 1
    if fault == "exact_ulp":
        bad = st.emulate(X, prec)
        k = int(np.argmax(np.abs(st.W32[:, last])))                     # the column's largest weight: one K index
        ulp = 2.0 ** (np.floor(np.log2(abs(float(st.W32[k, last])))) - 7)   # spacing of bf16 at that weight
        bad[:, last] += X[:, k] * ulp
        return bad
    if fault == "tile2_zero":
        bad = st.emulate(X, prec)
        bad[:, SECOND_TILE[name]] = 0.0
        return bad
    if fault == "unit_channel":
        cin = int(c[:, 3].max()) + 1
        assert (cin - 1) // L.CHAN_PAD == -(-cin // L.CHAN_PAD) - 1 and (cin - 1) % L.CHAN_PAD == 0   # alone in the last unit
        Xb = X.copy()
        Xb[:, c[:, 3] == cin - 1] = 0.0
        return st.emulate(Xb, prec)
    assert fault == "pad_leak"
    full = st.emulate(X, prec)
    Xb = X.copy()
    Xb[:, c[:, 2] == len(st.taps) // 2] = 0.0                             # the centre tap's rows of K
    full[:, last] = st.emulate(Xb, prec)[:, last]
    return full


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", EDGE_STAGES)
def test_edge_stage_emulation_passes_its_own_gate(name, prec):
    st, shape, vox, X, pre, S, g_acc, e_fmt, e_acc = _edge_setup(name, prec)
    print(f"{name} {prec}: K = {X.shape[1]}  e_fmt {e_fmt:.3e}  e_acc32 {e_acc:.3e}  g_acc {g_acc:.3e}")
    assert len(X) > L.M_TILE and len(X) % L.M_TILE
    ok, worst = _check(st, st.emulate(X, prec), pre, S, g_acc, prec)
    assert ok, L.describe(worst, vox, shape)
    if prec == "f32":
        ok, worst = _check(st, st.acc32_torch(X), pre, S, g_acc, prec)
        assert ok, L.describe(worst, vox, shape)
        acc, pre_s, S_s = st.acc32_sequential(X, prec, max_rows=1 << 30, max_cols=1 << 30)
        ok, worst = _check(st, acc, pre, S, g_acc, prec)
        assert ok, L.describe(worst, vox, shape)


@pytest.mark.parametrize("name,fault,prec", EDGE_FAULT_CASES)
def test_edge_fault_fails_the_gate(name, fault, prec):
    st, shape, vox, X, pre, S, g_acc, e_fmt, e_acc = _edge_setup(name, prec)
    ok, worst = _check(st, _edge_fault(st, X, prec, fault, name), pre, S, g_acc, prec)
    print(f"{name} {prec} {fault}: worst err/S {worst['max_err_over_S']:.3e} against g_acc {g_acc:.3e} (format {e_fmt:.3e}), "
          f"{L.describe(worst, vox, shape)}")
    assert not ok, f"{fault} passes the gate of {name} in {prec}: largest err/S {worst['max_err_over_S']:.3e}, g_acc {g_acc:.3e}"
    if fault in ("exact_ulp", "pad_leak"):
        assert worst["channel"] == st.cout - 1, worst           # and the message points at the column
    if fault == "tile2_zero":
        assert worst["channel"] == SECOND_TILE[name], worst


def test_one_bf16_ulp_of_one_product_is_inside_the_bf16_format():
    """The pair this comparison cannot separate at the exact-fit stage: in the bf16 mode every weight is rounded to bf16, half an
    ulp at the worst on each of the K = 1 728 products; one product of the last column off by a whole ulp is of that size, and
    stays under the gate that the format's own error sets.  f32 and the split mode refuse it (EDGE_FAULT_CASES)."""
    st, shape, vox, X, pre, S, g_acc, e_fmt, e_acc = _edge_setup("e64", "bf16")
    ok, worst = _check(st, _edge_fault(st, X, "bf16", "exact_ulp", "e64"), pre, S, g_acc, "bf16")
    print(f"one ulp of one product in bf16: err/S {worst['max_err_over_S']:.3e}, g_acc {g_acc:.3e}, format {e_fmt:.3e}")
    assert ok and worst["max_err_over_S"] < g_acc


def test_edge_net_shapes_keep_their_properties():
    """What the input shapes of tests/edge_nets.py were chosen for: every stage of E1 - E12 has more than one 256-row tile and a
    partial last one; the level-1 and decoder stages have overhanging and exact 4 x 4 tiles in y and in x; the counts of the table."""
    import edge_nets as E
    for tag in E.TAGS:
        convs = [o for o in L.walk(E.net_config(tag), E.shape_of(tag)) if o["type"] == "conv"]
        rows = [o["shape"][0] * o["shape"][1] * o["shape"][2] for o in convs]
        if tag != "E13":
            assert rows == E.STAGE_ROWS, (tag, rows)
            assert all(r > L.M_TILE and r % L.M_TILE for r in rows)
            ys, xs = {o["shape"][1] for o in convs[2:]}, {o["shape"][2] for o in convs[2:]}
            assert {v % 4 for v in ys} == {0, 2} and {v % 4 for v in xs} == {0, 2}, (ys, xs)
        else:
            assert (rows[5], rows[7], rows[9]) == (270, 240, 96), rows
        assert convs[-1]["shape"][3] <= 64      # the head's limit
    deepest = {tag: max(o["shape"][3] for o in L.walk(E.net_config(tag), E.shape_of(tag)) if o["type"] == "conv") for tag in E.TAGS}
    assert list(deepest.values()) == [64, 33, 65, 160, 161, 256, 304, 305, 320, 400, 480, 528, 640], deepest


@pytest.mark.parametrize("m", [2, 4])
def test_winograd_emulation_passes_and_clamp_fault_fails(m):
    """F(m x m) of the split mode on a 60-channel stage whose output extent (14 x 13) is no multiple of 4: the last tile row
    and column of F(4x4) overhang.  The fault: the last tile row reads clamped inputs one row too early."""
    prec = "bf16x3"
    rng = np.random.default_rng(4)
    shape = (5, 16, 15) if m == 4 else (5, 16, 14)
    x = _acts(rng, shape + (60,), prec)
    w, b = _weights(rng, 60, 60, (3, 3, 3))
    st = L.Stage([(L.Dense(x), (0, 0, 0), 60)], (3, 3, 3), w, b)
    oshape = tuple(s - 2 for s in shape) + (60,)
    vox = L.all_voxels(oshape)
    X = st.rows(*vox)
    pre, S = st.ref(X)
    emu = L.wino_emulate(x, w, m).reshape(-1, 60) + st.b
    e_fmt, e_acc = L.allowances(st, X, pre, S, prec, wino=True, emu_pre=emu)
    e_direct = L.norm_err(st.emulate(X, prec), pre, S)
    g_acc = L.gate(e_fmt, e_acc)
    print(f"F({m}x{m}): e_fmt {e_fmt:.3e} (direct split form {e_direct:.3e})  e_acc32 {e_acc:.3e}  g_acc {g_acc:.3e}")
    assert e_fmt < 50 * e_direct   # the transforms amplify the operand rounding, they do not lose the lo parts
    ok, worst = _check(st, emu, pre, S, g_acc, prec)
    assert ok, L.describe(worst, vox, oshape)
    bad = L.wino_emulate(x, w, m, clamp_rows=1).reshape(-1, 60) + st.b
    ok, worst = _check(st, bad, pre, S, g_acc, prec)
    assert not ok, f"clamped last tile row passes: err/S {worst['max_err_over_S']:.3e}, g_acc {g_acc:.3e}"
    y = vox[1][worst["row"]]
    assert y == oshape[1] - 1, L.describe(worst, vox, oshape)   # and the message points at the last row


def test_g_out_is_the_unit_roundoff_of_each_store():
    """g_out is derived from the formats: the worst relative error of a round-to-nearest-even store, reached at the ties just
    above a power of two.  bf16 has 8 significant bits: 2^-8 (not 2^-9, which its own correctly rounded store would miss)."""
    for prec, x in (("bf16", 1 + 2.0 ** -8), ("bf16x3", 1 + 2.0 ** -8 + 2.0 ** -17), ("f32", 1 + 2.0 ** -24)):
        got = float(L.store(np.array([x]), prec)[0])
        rel = abs(got - x) / x
        assert L.G_OUT[prec] / 2 < rel * (1 + 2.0 ** -7) and rel <= L.G_OUT[prec], (prec, rel, L.G_OUT[prec])
    rng = np.random.default_rng(1)
    v = rng.standard_normal(1 << 16) * np.exp(rng.uniform(-20, 20, 1 << 16))
    for prec in PRECS:
        rel = np.abs(L.store(v, prec).astype(np.float64) - v) / np.abs(v)
        assert L.G_OUT[prec] / 2 < rel.max() <= L.G_OUT[prec], (prec, rel.max())


def test_maxpool_of_split_values_takes_the_pair():
    """The pool of the split mode is the max of hi + lo; max(hi) and max(lo) taken separately is another number."""
    rng = np.random.default_rng(2)
    v = L.store(rng.standard_normal((4, 8, 8, 16)), "bf16x3")
    hi = L.bf16_rne(v)
    lo = v - hi
    ref = L.maxpool(v, (1, 2, 2))
    assert np.array_equal(L.store(ref, "bf16x3"), ref)           # a stored value: the pool adds no rounding, bit-equality is the gate
    bad = L.maxpool(hi, (1, 2, 2)) + L.maxpool(lo, (1, 2, 2))
    assert not np.array_equal(bad, ref)


def test_upsampled_tensor_matches_torch_trilinear():
    rng = np.random.default_rng(3)
    low = rng.standard_normal((3, 5, 6, 4))
    for f, o, shape in (((1, 2, 2), (0, 1, 2), (3, 8, 7, 4)), ((2, 2, 2), (1, 0, 1), (4, 10, 10, 4)), ((1, 3, 3), (0, 2, 1), (3, 11, 16, 4))):
        up = L.Upsampled(L.Dense(low), f, o, shape)
        t = torch.nn.functional.interpolate(torch.from_numpy(low.transpose(3, 0, 1, 2))[None], scale_factor=tuple(float(v) for v in f),
                                            mode="trilinear")[0].numpy().transpose(1, 2, 3, 0)
        want = t[o[0]:o[0] + shape[0], o[1]:o[1] + shape[1], o[2]:o[2] + shape[2]]
        assert np.abs(up.full() - want).max() < 1e-13
        vox = L.all_voxels(shape)
        assert np.abs(up.at(*vox).reshape(shape) - want).max() < 1e-13


def test_gemm_view_is_the_convolution():
    """Stage.rows / ref against torch's float64 conv3d, residual over a concatenation included."""
    st, shape = make_stage("rconv", "f32")
    vox = L.all_voxels(shape)
    pre, _ = st.ref(st.rows(*vox))
    f32 = L.conv3d_f32(st, shape)
    assert np.abs(pre.reshape(shape) - f32).max() < 1e-4 * np.abs(pre).max()
    skip, so, _ = st.src[0]
    up = st.src[1][0]
    x = np.concatenate([skip.full()[so[0]:so[0] + 5, so[1]:so[1] + 16, so[2]:so[2] + 14], up.full()], axis=3)
    xt = torch.from_numpy(x.transpose(3, 0, 1, 2))[None]
    nmain = int((st.cols[:, 0] == 0).sum())
    # float64 by torch: rebuild the OIDHW weights source by source
    blocks, row = [], 0
    for _, _, c in st.src:
        blocks.append(st.W[row:row + 27 * c].reshape(3, 3, 3, c, st.cout).transpose(4, 3, 0, 1, 2))
        row += 27 * c
    w64 = torch.from_numpy(np.ascontiguousarray(np.concatenate(blocks, axis=1)))
    out = torch.nn.functional.conv3d(xt, w64, torch.from_numpy(st.bias))
    wr = torch.from_numpy(np.ascontiguousarray(st.W[nmain:].T))[:, :, None, None, None]
    out = out + torch.nn.functional.conv3d(xt[:, :, 1:-1, 1:-1, 1:-1], wr, torch.from_numpy(st.bias_res))
    assert np.abs(out[0].numpy().transpose(1, 2, 3, 0) - pre.reshape(shape)).max() < 1e-12


def _family_config(golden_dir, tag):
    from test_oracle_unet import family_case
    return family_case(golden_dir, tag)


def test_walker_reproduces_output_shapes(golden_dir):
    """The plan walker on the full net and on family configs against bsmi_unet_output_shape (no GPU needed)."""
    from bootstrapper_amd.unet import Model
    from test_lib_cpu import AFFS_NET_CONFIG
    for nc, shape in ((AFFS_NET_CONFIG, (156, 220, 220)), (AFFS_NET_CONFIG, (124, 188, 188))):
        ops = L.walk(nc, shape)
        assert ops[-1]["type"] == "head" and ops[-1]["shape"][:3] == Model(nc).output_shape(shape)
        assert [o["type"] for o in ops].count("conv") == 14 and len(ops) == 1 + 14 + 3 + 3 + 1
    for tag in ("from_2d_mtlsd_f3i2", "2d_mtlsd_f4i2"):
        nc, sd, ins, x, refs = _family_config(golden_dir, tag)
        shape = x.shape[2:]
        ops = L.walk(nc, shape)
        heads = [o for o in ops if o["type"] == "head"]
        assert len(heads) == len(refs)
        want = Model(nc).output_shape(shape)
        for h, r in zip(heads, refs):
            assert h["shape"][:3] == want and h["shape"][3] == r.shape[0]
        # channel bookkeeping: every conv's sources add up to its weight's input channels
        for o in ops:
            if o["type"] == "conv":
                wkey = f"{o['prefix']}.conv_pass.{2 * o['conv']}.weight"
                assert sum(c for _, _, c in o["src"]) == sd[wkey].shape[1] and o["shape"][3] == sd[wkey].shape[0], wkey
