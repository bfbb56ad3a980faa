"""The first stage of a decoder ConvPass behind a fused (1,2,2) upsampling with its upsampled source convolved BELOW the
upsampling (csrc/unet_rules.hip below_up_site, csrc/wino.hip wino4_out_kernel<.., BELOW>): the skip connection stays in F(4x4)
form, the nine in-plane taps of the upsampled source are nine (3,1,1) GEMM column groups over the low-resolution tensor, and
the output transform interpolates and adds them.  BSMI_CONV_BELOW_UP=0 restores the F(4x4) form over both sources,
BSMI_FUSE_UP=0 turns every fusion off.  Needs an MI355X; every switch is read once per process, so each configuration runs in
a child process.

Nets: A (14, 52, 52) and B (14, 60, 60, odd crop offset) of tests/test_fuse_up_narrow_gpu.py, restated here, and C_NET of
tests/test_layers_gpu.py at (22, 116, 116): its 360 -> 60 pass has the real channel counts of the narrow stage, overhanging
tiles (42 x 42) and a ragged last row tile.  These three have at most 64 output channels: the nine taps side by side as
columns of one GEMM.  E is C_NET with 16 / 80 / 400 feature maps at (22, 60, 60): its lower decoder pass is 480 -> 80 at
14 x 14 (2 mod 4), more than 64 output channels: the nine taps as nine batches.

Checks:
  values  every step of the forward against float64 within the bounds of tests/layer_ref.py (test_layers_gpu.run_case), in
          every configuration.
  plan    plan_steps() reports below_up exactly on the stages the rule names (RULE below restates it) and nowhere with the
          switch off or without the fusion; form and flags of those stages stay "winograd F(4x4)" / fused-up.
  rules   the pass's first activation under two rules differs by at most the sum of their two layer_ref bounds, element-wise
          (a rule's bound: g_acc S + g_out |ref| of that step, from the reference alone).
  bits    two default forwards give equal bits.
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
C_NET = {"in_channels": 1, "num_fmaps": 12, "fmap_inc_factor": 5, "downsample_factors": [[1, 2, 2], [1, 2, 2]],
         "kernel_size_down": [K3] * 3, "kernel_size_up": [K3] * 2, "outputs": {"3d_affs": {"dims": 6}}}
# net, input shape, weight seed, input seed, the pass under test, its (cin of the upsampled source, cout)
NETS = {
    "A": ({"in_channels": 1, "num_fmaps": 64, "fmap_inc_factor": 4, "downsample_factors": [[1, 2, 2]],
           "kernel_size_down": [K3, K3], "kernel_size_up": [K3], "outputs": {"3d_affs": {"dims": 6}}}, (14, 52, 52), 5, 11, "unet.r_conv.0.0", (256, 64)),
    "B": ({"in_channels": 1, "num_fmaps": 64, "fmap_inc_factor": 3, "downsample_factors": [[1, 2, 2], [1, 3, 3]],
           "kernel_size_down": [K3, K3, K1], "kernel_size_up": [K3, K1], "outputs": {"3d_affs": {"dims": 6}}}, (14, 60, 60), 5, 11, "unet.r_conv.0.0", (192, 64)),
    "C": (C_NET, (22, 116, 116), 3, 7, "unet.r_conv.0.1", (300, 60)),
    "E": (dict(C_NET, num_fmaps=16), (22, 60, 60), 5, 11, "unet.r_conv.0.1", (400, 80)),
}
CONFIGS = {"default": {}, "below-off": {"BSMI_CONV_BELOW_UP": "0"}, "fuse-off": {"BSMI_FUSE_UP": "0"}}
_DEAD = (134, 139, 124, 137, -6, -11, -9)
_STOP = []


def RULE(cin_low, cout):
    """csrc/unet_rules.hip below_up_site, the default rule: which first stages behind a fused upsampling take the form"""
    return True


def _case(tag):
    from bootstrapper_amd.synth import synthetic_state_dict
    nc, shape, wseed, rseed, _, _ = NETS[tag]
    raw = np.random.default_rng(rseed).integers(0, 256, size=shape, dtype=np.uint8)
    return nc, synthetic_state_dict(nc, wseed), raw


# ---- child process: one configuration --------------------------------------------------------------------------------------
def _child_main(tag, out_path):
    import torch
    import layer_ref as L
    import test_layers_gpu as T
    from bootstrapper_amd.unet import Model
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    prec = "bf16x3"
    nc, sd, raw = _case(tag)
    PASS = NETS[tag][4]
    T.run_case(f"below-up:{tag}", nc, sd, raw, prec, record=T.Record())   # every step within its layer_ref bound

    m = Model(nc, precision=prec).load_state_dict(sd)
    x = torch.from_numpy(raw).cuda()
    u8a, f32a = m.predict_u8(x, want_f32=True)
    torch.cuda.synchronize()
    out = f32a[0].cpu().numpy()
    plan = m.plan_steps()
    ops = L.walk(nc, raw.shape)
    L.check_walk(ops, plan)
    convs = [i for i, o in enumerate(ops) if o["type"] == "conv" and o["prefix"] == PASS]
    first = convs[0]
    got = m.debug_activation(first)
    u8b, f32b = m.predict_u8(x, want_f32=True)
    torch.cuda.synchronize()
    same_bits = bool(np.array_equal(out.view(np.uint32), f32b[0].cpu().numpy().view(np.uint32)) and torch.equal(u8a[0], u8b[0]) and
                     np.array_equal(got.view(np.uint32), m.debug_activation(first).view(np.uint32)))
    iu = [s for s, _, _ in ops[first]["src"] if ops[s]["type"] == "up"][0]
    info = {"up_materialised": plan[iu]["materialised"], "up_offset": list(ops[iu]["offset"]),
            "first": [plan[first]["form"], list(plan[first]["flags"])], "shape": list(ops[first]["shape"]),
            "below_up": {f"{p['prefix']}:{p['conv']}": bool(p["below_up"]) for p in plan if p["type"] == "conv"}, "same_bits": same_bits}

    # the pass's first activation: float64 reference on the step's own inputs as the device holds them, and its bound
    def tensor(s):
        if plan[s]["materialised"]:
            return L.Dense(m.debug_activation(s))
        o = ops[s]
        return L.Upsampled(L.Dense(m.debug_activation(o["src"])), o["factor"], o["offset"], o["shape"])

    o, p = ops[first], plan[first]
    shape = tuple(o["shape"])
    src = [(tensor(s), org, c) for s, org, c in o["src"]]
    key = f"{PASS}.conv_pass.{2 * o['conv']}"
    st = L.Stage(src, o["kernel"], T._w5(sd[key + ".weight"]), sd[key + ".bias"], None, None, None)
    vox = L.all_voxels(shape)
    X = st.rows(*vox)
    pre, S = st.ref(X)
    wino_m = {"winograd F(2x2)": 2, "winograd F(4x4)": 4}.get(p["form"], 0)
    emu = None
    if wino_m:
        full = L.wino_emulate(T._block_input(src, (0, shape[0] + 2), (0, shape[1] + 2), (0, shape[2] + 2)), T._w5(sd[key + ".weight"]), wino_m)
        emu = full[vox] + st.bias
    e_fmt, e_acc = L.allowances(st, X, pre, S, prec, bool(wino_m), "split-k" in p["flags"], emu_pre=emu, f32_pre=L.conv3d_f32(st, shape)[vox])
    g_acc = L.gate(e_fmt, e_acc)
    ref = st.act(pre)
    bound = g_acc * S + L.G_OUT[prec] * np.abs(ref)
    err = np.abs(got[vox].astype(np.float64) - ref)
    info.update(g_acc=g_acc, act_max_err_over_bound=float((err / np.maximum(bound, 1e-300)).max()), act_max_err=float(err.max()))
    print("BELOW-UP-INFO " + json.dumps(info))
    np.savez(out_path, act=got[vox], bound=bound, info=json.dumps(info))
    assert np.all(err <= bound), info


# ---- parent ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs():
    """{(net, configuration): npz} -- every child runs once, the tests share the results."""
    cache = {}
    tmp = tempfile.TemporaryDirectory()
    drop = ("BSMI_CONV_BELOW_UP", "BSMI_FUSE_UP_NARROW", "BSMI_FUSE_UP", "BSMI_WINO", "BSMI_WINO4", "BSMI_H16")

    def get(tag, cfg):
        if (tag, cfg) in cache:
            return cache[(tag, cfg)]
        if _STOP:
            pytest.skip(f"a child process died earlier ({_STOP[0]}): no further GPU work in this run")
        path = os.path.join(tmp.name, f"{tag}_{cfg}.npz")
        env = {k: v for k, v in os.environ.items() if k not in drop}
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), tag, path], env=dict(env, **CONFIGS[cfg]), capture_output=True, text=True,
                               timeout=300, cwd=ROOT)
        except subprocess.TimeoutExpired:
            _STOP.append(f"{tag} {cfg}: timeout")
            raise
        if r.returncode in _DEAD:
            _STOP.append(f"{tag} {cfg}: exit status {r.returncode}")
        print("\n".join(l for l in r.stdout.splitlines() if l.startswith("BELOW-UP-INFO") or (" conv 0 " in l and NETS[tag][4] in l)))
        assert r.returncode == 0, f"{tag} {cfg}:\n" + r.stdout[-6000:] + r.stderr[-3000:]
        d = np.load(path)
        cache[(tag, cfg)] = dict(act=d["act"], bound=d["bound"], info=json.loads(str(d["info"])))
        return cache[(tag, cfg)]
    yield get
    tmp.cleanup()


@pytest.mark.parametrize("tag", sorted(NETS))
def test_default_rule_names_the_stages(runs, tag):
    """(the child has also checked every step of the forward against float64 within layer_ref's bounds)"""
    info = runs(tag, "default")["info"]
    key = NETS[tag][4] + ":0"
    want = RULE(*NETS[tag][5])
    assert info["up_materialised"] is False, info
    assert info["first"][0] == "winograd F(4x4)" and "fused-up" in info["first"][1], info
    assert info["below_up"][key] is want, info
    assert [k for k, v in info["below_up"].items() if v] == ([key] if want else []), info
    if tag == "B":
        assert tuple(info["up_offset"]) == (0, 1, 1), info
    if tag == "A":
        assert info["shape"][1:3] == [38, 38], info
    if tag == "E":
        assert info["shape"][1:] == [14, 14, 80], info


@pytest.mark.parametrize("cfg", ["below-off", "fuse-off"])
@pytest.mark.parametrize("tag", sorted(NETS))
def test_switches_turn_the_form_off(runs, tag, cfg):
    info = runs(tag, cfg)["info"]
    assert not any(info["below_up"].values()), info
    assert info["up_materialised"] is (cfg == "fuse-off"), info
    assert info["first"][0] == "winograd F(4x4)" and ("fused-up" in info["first"][1]) is (cfg == "below-off"), info


@pytest.mark.parametrize("cfg", ["below-off", "fuse-off"])
@pytest.mark.parametrize("tag", sorted(NETS))
def test_rules_agree_within_the_sum_of_their_bounds(runs, tag, cfg):
    a, b = runs(tag, "default"), runs(tag, cfg)
    bsum = a["bound"] + b["bound"]
    d = np.abs(a["act"].astype(np.float64) - b["act"].astype(np.float64))
    print(f"{tag} default vs {cfg}: first activation max |diff| {d.max():.3e}, largest diff / (sum of bounds) {(d / np.maximum(bsum, 1e-300)).max():.3e}")
    assert np.all(d <= bsum)


@pytest.mark.parametrize("tag", sorted(NETS))
def test_two_default_forwards_give_equal_bits(runs, tag):
    assert runs(tag, "default")["info"]["same_bits"] is True


if __name__ == "__main__":
    _child_main(sys.argv[1], sys.argv[2])
