"""The decoder rule of csrc/unet_rules.hip wino_narrow_last: behind a (1,2,2) upsampling the narrow last stage of a decoder
ConvPass takes the Winograd form whenever the pass's first stage does, so that Planner::rec fuses the upsampling into the pass
(the map is never written).  BSMI_FUSE_UP_NARROW=0 restores the rule before it, BSMI_FUSE_UP=0 turns every fusion off.  Needs
an MI355X; every switch is read once per process, so each configuration runs in a child process.

Nets (channels chosen so that the pass's first stage is a Winograd stage by its own cin * cout >= 16 384 and its last stage,
cout^2 < 16 384, is not):
  A  two levels, 64 / 256 feature maps, one (1,2,2) level, 3x3x3 kernels, input (14, 52, 52): the decoder pass is 320 -> 64 at
     38 x 38 (= 2 mod 4: overhanging F(4x4) tiles), then 64 -> 64 at 36 x 36; the upsampling is cropped by (0, 0, 0).
  B  three levels, 64 / 192 / 576 feature maps, input (14, 60, 60); the pass under test is the top decoder pass, 256 -> 64 then
     64 -> 64, behind the (1,2,2) upsampling, whose map is cropped by the ODD offset (0, 1, 1): the input transform's
     <PY, PX> = <1, 1> form.  With (1,2,2) factors and 3x3x3 kernels on every level no input gives an odd offset (the extent
     below an upsampling is 2 h - 4, even, so the map's extent is a multiple of 4 = the crop factor), and three levels of 3x3x3
     passes need 21 planes: so the level below pools by (1,3,3) (crop factor (1,6,6) on top) and the two passes at the bottom
     have (1,3,3) kernels.  (14, 60, 60) is the smallest input of this net with the odd offset in y and x.

Checks, for both nets:
  plan    default rule: the pass's UP step is not materialised (debug_activation refuses it), both of its conv steps report
          winograd F(4x4) with fused-up, the last also res-low.  BSMI_FUSE_UP_NARROW=0 and BSMI_FUSE_UP=0: the step is
          materialised, the first stage is F(4x4) without flags and the last stage is not a Winograd stage.
  values  every step of the forward against float64 within the bounds of tests/layer_ref.py (test_layers_gpu.run_case: that
          includes the last decoder activation and the head outputs), in every configuration.
  rules   the last decoder activation of two rules differs by at most the sum of their two bounds, element-wise, where a rule's
          bound is layer_ref's g_acc S + g_out |ref| of that step (g_acc from the emulation of the step's own form: no figure
          of the code under test enters).  The outputs differ by at most that sum carried through the head -- a 1x1x1
          convolution with weights w1 + w2, then a sigmoid, whose slope is at most 1/4 -- plus the head kernel's own gate for
          either side:  |out_a - out_b| <= 2 G_HEAD + (b_a + b_b) |w1 + w2|^T / 4.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

K3 = [[3, 3, 3], [3, 3, 3]]
K1 = [[1, 3, 3], [1, 3, 3]]
NETS = {
    "A": ({"in_channels": 1, "num_fmaps": 64, "fmap_inc_factor": 4, "downsample_factors": [[1, 2, 2]],
           "kernel_size_down": [K3, K3], "kernel_size_up": [K3], "outputs": {"3d_affs": {"dims": 6}}}, (14, 52, 52), (0, 0, 0)),
    "B": ({"in_channels": 1, "num_fmaps": 64, "fmap_inc_factor": 3, "downsample_factors": [[1, 2, 2], [1, 3, 3]],
           "kernel_size_down": [K3, K3, K1], "kernel_size_up": [K3, K1], "outputs": {"3d_affs": {"dims": 6}}}, (14, 60, 60), (0, 1, 1)),
}
CONFIGS = {"default": {}, "narrow-off": {"BSMI_FUSE_UP_NARROW": "0"}, "fuse-off": {"BSMI_FUSE_UP": "0"}}
PASS = "unet.r_conv.0.0"   # the top decoder pass: the one behind the (1,2,2) upsampling in both nets
_DEAD = (134, 139, 124, 137, -6, -11, -9)
_STOP = []


def _case(tag):
    from bootstrapper_amd.synth import synthetic_state_dict
    nc, shape, _ = NETS[tag]
    raw = np.random.default_rng(11).integers(0, 256, size=shape, dtype=np.uint8)
    return nc, synthetic_state_dict(nc, 5), raw


# ---- child process: one configuration --------------------------------------------------------------------------------------
def _child_main(tag, out_path):
    import torch
    import layer_ref as L
    import test_layers_gpu as T
    from bootstrapper_amd.unet import Model
    from bootstrapper_amd._lib import BsmiError, ERR_STATE
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    prec = "bf16x3"
    nc, sd, raw = _case(tag)
    T.run_case(f"narrow:{tag}", nc, sd, raw, prec, record=T.Record())   # every step within its layer_ref bound

    m = Model(nc, precision=prec).load_state_dict(sd)
    _, f32 = m.predict_u8(torch.from_numpy(raw).cuda(), want_f32=True)
    torch.cuda.synchronize()
    out = f32[0].cpu().numpy()
    plan = m.plan_steps()
    ops = L.walk(nc, raw.shape)
    L.check_walk(ops, plan)
    convs = [i for i, o in enumerate(ops) if o["type"] == "conv" and o["prefix"] == PASS]
    first, last = convs[0], convs[-1]
    iu = [s for s, _, _ in ops[first]["src"] if ops[s]["type"] == "up"][0]
    info = {"up_materialised": plan[iu]["materialised"], "up_offset": list(ops[iu]["offset"]), "up_factor": list(ops[iu]["factor"]),
            "first": [plan[first]["form"], list(plan[first]["flags"])], "last": [plan[last]["form"], list(plan[last]["flags"])],
            "shapes": [list(ops[first]["shape"]), list(ops[last]["shape"])]}
    if not plan[iu]["materialised"]:
        try:
            m.debug_activation(iu)
            info["up_refused"] = False
        except BsmiError as e:
            info["up_refused"] = e.code == ERR_STATE and "not materialised" in e.msg

    # the last decoder activation: float64 reference on the step's own inputs as the device holds them, and its bound
    def tensor(s):
        if plan[s]["materialised"]:
            return L.Dense(m.debug_activation(s))
        o = ops[s]
        return L.Upsampled(L.Dense(m.debug_activation(o["src"])), o["factor"], o["offset"], o["shape"])

    o, p = ops[last], plan[last]
    got = m.debug_activation(last)
    shape = tuple(o["shape"])
    src = [(tensor(s), org, c) for s, org, c in o["src"]]
    res = [(tensor(s), org, c) for s, org, c in o["res"]]
    key = f"{PASS}.conv_pass.{2 * o['conv']}"
    st = L.Stage(src, o["kernel"], T._w5(sd[key + ".weight"]), sd[key + ".bias"], res, T._w5(sd[PASS + ".residual.0.weight"]), sd[PASS + ".residual.0.bias"])
    vox = L.all_voxels(shape)
    X = st.rows(*vox)
    pre, S = st.ref(X)
    wino_m = {"winograd F(2x2)": 2, "winograd F(4x4)": 4}.get(p["form"], 0)
    emu = None
    if wino_m:
        full = L.wino_emulate(T._block_input(src, (0, shape[0] + 2), (0, shape[1] + 2), (0, shape[2] + 2)), T._w5(sd[key + ".weight"]), wino_m)
        emu = full[vox] + st.bias + st.emulate(X, prec, part="res")
    e_fmt, e_acc = L.allowances(st, X, pre, S, prec, bool(wino_m), "split-k" in p["flags"], emu_pre=emu, f32_pre=L.conv3d_f32(st, shape)[vox])
    g_acc = L.gate(e_fmt, e_acc)
    ref = st.act(pre)
    bound = g_acc * S + L.G_OUT[prec] * np.abs(ref)
    err = np.abs(got[vox].astype(np.float64) - ref)
    info.update(g_acc=g_acc, e_fmt=e_fmt, e_acc32=e_acc, act_max_err_over_bound=float((err / np.maximum(bound, 1e-300)).max()), act_max_err=float(err.max()))
    print("NARROW-INFO " + json.dumps(info))
    np.savez(out_path, act=got[vox], bound=bound, out=out, info=json.dumps(info))
    assert np.all(err <= bound), info


# ---- parent ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs():
    """{(net, configuration): npz} -- every child runs once, the tests share the results."""
    cache = {}
    tmp = tempfile.TemporaryDirectory()

    def get(tag, cfg):
        if (tag, cfg) in cache:
            return cache[(tag, cfg)]
        if _STOP:
            pytest.skip(f"a child process died earlier ({_STOP[0]}): no further GPU work in this run")
        path = os.path.join(tmp.name, f"{tag}_{cfg}.npz")
        env = {k: v for k, v in os.environ.items() if k not in ("BSMI_FUSE_UP_NARROW", "BSMI_FUSE_UP", "BSMI_WINO", "BSMI_WINO4", "BSMI_H16")}
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), tag, path], env=dict(env, **CONFIGS[cfg]), capture_output=True, text=True,
                               timeout=300, cwd=ROOT)
        except subprocess.TimeoutExpired:
            _STOP.append(f"{tag} {cfg}: timeout")
            raise
        if r.returncode in _DEAD:
            _STOP.append(f"{tag} {cfg}: exit status {r.returncode}")
        print("\n".join(l for l in r.stdout.splitlines() if l.startswith("NARROW-INFO") or " conv " in l))
        assert r.returncode == 0, f"{tag} {cfg}:\n" + r.stdout[-6000:] + r.stderr[-3000:]
        d = np.load(path)
        cache[(tag, cfg)] = dict(act=d["act"], bound=d["bound"], out=d["out"], info=json.loads(str(d["info"])))
        return cache[(tag, cfg)]
    yield get
    tmp.cleanup()


@pytest.mark.parametrize("tag", ["A", "B"])
def test_default_rule_fuses_the_upsampling(runs, tag):
    """(the child has also checked every step of the forward against float64 within layer_ref's bounds)"""
    info = runs(tag, "default")["info"]
    assert info["up_factor"] == [1, 2, 2] and tuple(info["up_offset"]) == NETS[tag][2], info
    assert info["up_materialised"] is False and info["up_refused"] is True, info
    assert info["first"][0] == "winograd F(4x4)" and "fused-up" in info["first"][1], info
    assert info["last"][0] == "winograd F(4x4)" and {"fused-up", "res-low"} <= set(info["last"][1]), info
    if tag == "A":
        assert [s[1:3] for s in info["shapes"]] == [[38, 38], [36, 36]], info


@pytest.mark.parametrize("cfg", ["narrow-off", "fuse-off"])
@pytest.mark.parametrize("tag", ["A", "B"])
def test_switches_restore_the_materialised_map(runs, tag, cfg):
    info = runs(tag, cfg)["info"]
    assert info["up_materialised"] is True, info
    assert info["first"] == ["winograd F(4x4)", []], info
    assert not info["last"][0].startswith("winograd") and "fused-up" not in info["last"][1] and "res-low" not in info["last"][1], info


@pytest.mark.parametrize("cfg", ["narrow-off", "fuse-off"])
@pytest.mark.parametrize("tag", ["A", "B"])
def test_rules_agree_within_the_sum_of_their_bounds(runs, tag, cfg):
    from test_layers_gpu import G_HEAD, _w5
    a, b = runs(tag, "default"), runs(tag, cfg)
    bsum = a["bound"] + b["bound"]
    d = np.abs(a["act"].astype(np.float64) - b["act"].astype(np.float64))
    print(f"{tag} default vs {cfg}: last decoder activation max |diff| {d.max():.3e}, largest diff / (sum of bounds) {(d / np.maximum(bsum, 1e-300)).max():.3e}")
    assert np.all(d <= bsum)
    _, sd, _ = _case(tag)
    w = (_w5(sd["affs_head.conv_pass.0.weight"]) + _w5(sd["affs_head.residual.0.weight"]))[:, :, 0, 0, 0].astype(np.float64)   # (6, C)
    obound = 2 * G_HEAD + 0.25 * bsum @ np.abs(w).T                                                        # (voxels, 6)
    od = np.abs(a["out"].astype(np.float64) - b["out"].astype(np.float64)).reshape(w.shape[0], -1).T
    print(f"{tag} default vs {cfg}: output max |diff| {od.max():.3e}, largest diff / bound {(od / obound).max():.3e}")
    assert np.all(od <= obound)


if __name__ == "__main__":
    _child_main(sys.argv[1], sys.argv[2])
