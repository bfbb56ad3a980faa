"""Winograd stages that are F(2,3) along z as well as F(4x4) in (y, x) -- the "wz" form (csrc/unet_rules.hip wino_z_site,
csrc/wino.hip wino4_in_kernel<true> / wino4z_out_kernel, tests/wino_z_ref.py).  BSMI_WINO_Z=1 sends every stage the kernels can
take through it, 0 none, unset the rule (the widest stages only: none of the nets here).  Needs an MI355X; the switches are read
once per process, so each configuration runs in a child process.

Nets: a (1,3,3) encoder pass, a (1,2,2) pooling, a 3x3x3 bottom pass whose two stages are the stages under test (the second
one carries the pass's 1x1x1 residual addend), a (1,3,3) decoder pass.  The bottom pass's input is 8 x 10 x 10 (even Do, whole
tiles) or 9 x 12 x 12 (Do = 7, 10 x 10 outputs: an overhanging pair and overhanging tiles):
  P1  20 -> 80 -> 80    Cin 20: pad channels inside a 32-channel chunk            even
  P2  24 -> 72 -> 72    Cin 72: an odd number of 16-channel units, the dummy unit  odd
  P3  12 -> 24 -> 24    Cout 24, the narrow tile                                    odd
  P4  24 -> 264 -> 264  Cout 264, the wide tile                                     even
(the tile each Cout runs on is the launcher's choice and printed with the plan.)  K is a net in which no stage can take the form
under BSMI_WINO_Z=1: its 3x3x3 stages are the last stage of an encoder pass with fused pooling and the first and last stage of a
decoder pass behind a fused upsampling.

Checks:
  values   every step of the forward against float64 within the bounds of tests/layer_ref.py (test_layers_gpu.run_case), with
           the wz emulation as `emu_pre` of layer_ref.allowances on the stages that plan_steps() reports with wino_z
  plan     wino_z exactly on the bottom pass's two stages; nowhere in K, whose stages keep "winograd F(4x4)" with their fusions
  bits     K under BSMI_WINO_Z=1 and =0, P2 under =0 and unset, P2 with host-packed and device-packed weights: equal hashes of
           every activation and of the heads' outputs
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

K3 = [[3, 3, 3], [3, 3, 3]]
K1 = [[1, 3, 3], [1, 3, 3]]
EVEN, ODD = (8, 24, 24), (9, 28, 28)   # the bottom pass's input: 8 x 10 x 10, 9 x 12 x 12


def _pnet(nf, inc):
    return {"in_channels": 1, "num_fmaps": nf, "fmap_inc_factor": inc, "downsample_factors": [[1, 2, 2]], "kernel_size_down": [K1, K3],
            "kernel_size_up": [K1], "outputs": {"3d_affs": {"dims": 6}}}


NETS = {
    "P1": (_pnet(20, 4), EVEN),
    "P2": (_pnet(24, 3), ODD),
    "P3": (_pnet(12, 2), ODD),
    "P4": (_pnet(24, 11), EVEN),
    "K": ({"in_channels": 1, "num_fmaps": 32, "fmap_inc_factor": 2, "downsample_factors": [[1, 2, 2]],
           "kernel_size_down": [[[1, 3, 3], [3, 3, 3]], K1], "kernel_size_up": [K3], "outputs": {"3d_affs": {"dims": 6}}}, (12, 28, 28)),
}
FORCE = {"BSMI_WINO": "2"}
CONFIGS = {
    "wz": dict(FORCE, BSMI_WINO_Z="1"),
    "wz-host-pack": dict(FORCE, BSMI_WINO_Z="1", BSMI_WINO_PACK_HOST="1"),
    "off": dict(FORCE, BSMI_WINO_Z="0"),
    "rule": dict(FORCE),
}
_DEAD = (134, 139, 124, 137, -6, -11, -9)
_STOP = []


def _case(tag):
    from bootstrapper_amd.synth import synthetic_state_dict
    nc, shape = NETS[tag]
    raw = np.random.default_rng(11).integers(0, 256, size=shape, dtype=np.uint8)
    return nc, synthetic_state_dict(nc, 5), raw


# ---- child process: one configuration --------------------------------------------------------------------------------------
def _child_main(tag, check):
    import torch
    import layer_ref as L
    import wino_z_ref as Z
    import test_layers_gpu as T
    from bootstrapper_amd.unet import Model
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    nc, sd, raw = _case(tag)
    if check:
        # run_case asks layer_ref.wino_emulate for the emulation of a Winograd step: a step that runs the wz form gets the wz emulation
        state = {"wz": False}
        plain_emulate, plain_check = L.wino_emulate, T._check_conv

        def emulate(x, w, m, clamp_rows=0):
            return Z.wino_z_emulate(x, w, clamp_rows) if state["wz"] else plain_emulate(x, w, m, clamp_rows)

        def check_conv(case, prec, i, o, p, *rest):
            state["wz"] = bool(p["wino_z"])
            assert not state["wz"] or p["form"] == "winograd F(4x4)", p
            return plain_check(case, prec, i, o, p, *rest)

        L.wino_emulate, T._check_conv = emulate, check_conv
        T.run_case(f"wino-z:{tag}", nc, sd, raw, "bf16x3", record=T.Record())
    m = Model(nc, precision="bf16x3").load_state_dict(sd)
    u8, f32 = m.predict_u8(torch.from_numpy(raw).cuda(), want_f32=True)
    torch.cuda.synchronize()
    plan = m.plan_steps()
    hashes = {str(p["step"]): hashlib.sha256(m.debug_activation(p["step"]).tobytes()).hexdigest()
              for p in plan if p["materialised"] and p["type"] != "head"}
    hashes["f32"] = hashlib.sha256(f32[0].cpu().numpy().tobytes()).hexdigest()
    hashes["u8"] = hashlib.sha256(u8[0].cpu().numpy().tobytes()).hexdigest()
    convs = [dict(prefix=p["prefix"], conv=p["conv"], form=p["form"], flags=list(p["flags"]), wino_z=bool(p["wino_z"]), bn=p["bn"],
                  ksteps=p["ksteps"], shape=list(p["shape"])) for p in plan if p["type"] == "conv"]
    pools = [dict(step=p["step"], materialised=p["materialised"]) for p in plan if p["type"] in ("pool", "up")]
    print("WINO-Z-INFO " + json.dumps(dict(convs=convs, pools=pools, hashes=hashes)))


# ---- parent ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs():
    """{(net, configuration): info} -- every child runs once, the tests share the results."""
    cache = {}
    drop = ("BSMI_WINO_Z", "BSMI_WINO_PACK_HOST", "BSMI_CONV_BELOW_UP", "BSMI_FUSE_UP_NARROW", "BSMI_FUSE_UP", "BSMI_POOL_FUSE", "BSMI_WINO",
            "BSMI_WINO4", "BSMI_H16")

    def get(tag, cfg, check=False):
        if (tag, cfg) in cache:
            return cache[(tag, cfg)]
        if _STOP:
            pytest.skip(f"a child process died earlier ({_STOP[0]}): no further GPU work in this run")
        env = {k: v for k, v in os.environ.items() if k not in drop}
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), tag, "check" if check else "hash"], env=dict(env, **CONFIGS[cfg]),
                               capture_output=True, text=True, timeout=300, cwd=ROOT)
        except subprocess.TimeoutExpired:
            _STOP.append(f"{tag} {cfg}: timeout")
            raise
        if r.returncode in _DEAD:
            _STOP.append(f"{tag} {cfg}: exit status {r.returncode}")
        print("\n".join(l for l in r.stdout.splitlines() if " conv " in l and "step" in l))
        assert r.returncode == 0, f"{tag} {cfg}:\n" + r.stdout[-6000:] + r.stderr[-3000:]
        line = [l for l in r.stdout.splitlines() if l.startswith("WINO-Z-INFO ")][-1]
        cache[(tag, cfg)] = json.loads(line[len("WINO-Z-INFO "):])
        return cache[(tag, cfg)]
    return get


@pytest.mark.parametrize("tag", ["P1", "P2", "P3", "P4"])
def test_forced_form_within_the_layer_bounds(runs, tag):
    """(the child has checked every step of the forward against float64 within layer_ref's bounds, the wz steps with the wz emulation)"""
    info = runs(tag, "wz", check=True)
    nf, inc = NETS[tag][0]["num_fmaps"], NETS[tag][0]["fmap_inc_factor"]
    bottom = [c for c in info["convs"] if c["prefix"] == "unet.l_conv.1"]
    assert [c["wino_z"] for c in bottom] == [True, True] and all(c["form"] == "winograd F(4x4)" for c in bottom), info["convs"]
    assert [c["prefix"] + ":" + str(c["conv"]) for c in info["convs"] if c["wino_z"]] == ["unet.l_conv.1:0", "unet.l_conv.1:1"], info["convs"]
    do = 6 if NETS[tag][1] == EVEN else 7
    assert bottom[0]["shape"] == [do, 8 if do == 6 else 10, 8 if do == 6 else 10, nf * inc], bottom
    # K = channels only: one K-step per 32-channel chunk of V, padded to an even count
    for c, cin in zip(bottom, (nf, nf * inc)):
        chunks = -(-(-(-cin // 16) * 16) // 32)
        assert c["ksteps"] == chunks + (chunks & 1), (c, cin)
    print(tag, [(c["prefix"], c["conv"], c["bn"], c["ksteps"]) for c in bottom])


def test_stages_with_fusions_keep_the_plain_form(runs):
    on, off = runs("K", "wz", check=True), runs("K", "off")
    assert not any(c["wino_z"] for c in on["convs"]), on["convs"]
    by = {(c["prefix"], c["conv"]): c for c in on["convs"]}
    assert by[("unet.l_conv.0", 1)]["form"] == "winograd F(4x4)"                       # the encoder stage before the fused pooling
    for ci in (0, 1):                                                                 # the decoder pass behind the fused upsampling
        c = by[("unet.r_conv.0.0", ci)]
        assert c["form"] == "winograd F(4x4)" and "fused-up" in c["flags"], c
    assert [p for p in on["pools"] if not p["materialised"]], on["pools"]            # the upsampled map is not written
    assert on["convs"] == off["convs"] and on["hashes"] == off["hashes"]


def test_device_packed_weights_equal_host_packed(runs):
    dev, host = runs("P2", "wz", check=True), runs("P2", "wz-host-pack")
    assert dev["convs"] == host["convs"] and dev["hashes"] == host["hashes"]


def test_switch_off_equals_the_rule_where_it_selects_nothing(runs):
    off, rule = runs("P2", "off"), runs("P2", "rule")
    assert not any(c["wino_z"] for c in off["convs"]) and not any(c["wino_z"] for c in rule["convs"])
    assert off["convs"] == rule["convs"] and off["hashes"] == rule["hashes"]
    assert off["hashes"] != runs("P2", "wz", check=True)["hashes"]                  # ... and the forced form is another arithmetic


if __name__ == "__main__":
    _child_main(sys.argv[1], sys.argv[2] == "check")
