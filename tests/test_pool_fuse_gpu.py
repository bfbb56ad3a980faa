"""The pooled output of the F(4x4) output transform (csrc/wino.hip wino4_out_kernel<false, true>, WinoOutArgs::pool): a (1,2,2)
max-pool of even extents directly behind an F(4x4) stage is stored by that stage's output transform and the POOL step launches
nothing.  BSMI_POOL_FUSE=0 restores the separate launch.  The two must agree bit for bit: the hashes of every materialised
activation and of the outputs are compared.  Needs an MI355X; the switches are read once per process, so each configuration
runs in a child process.

Nets: two levels, 20 / 40 feature maps (20 channels are padded to 32: the pad channels are pooled like the others; more than 16,
so that the first ConvPass is not the first_pass launch), BSMI_WINO=2 so that the stage before the pool is an F(4x4) stage.
  mult4     input (14, 20, 20), pool (1,2,2) of a 16 x 16 map: whole tiles
  overhang  input (14, 22, 22), pool (1,2,2) of an 18 x 18 map (= 2 mod 4): the last tile row / column overhangs, its pooled
            outputs past the extent must not be stored (a store past the 9 x 9 map would land in the next row / plane and change
            the hash)
  factor3   input (14, 28, 28), pool (1,3,3) of a 24 x 24 map: must keep its own launch
  factor222 input (18, 20, 20), pool (2,2,2) of a (14, 16, 16) map: must keep its own launch
The raw input is constant on its left third (every window of the map there holds four equal values: ties), 4 x 4 blocks in the
middle and noise on the right; the synthetic weights leave about half of the values at zero after the ReLU, so windows of
zeros and windows with one or two zeros occur (the child counts and asserts both).
Whether the POOL step launched is read from the profile's launch counts (bsmi_unet_profile_totals)."""
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


def _net(factor):
    return {"in_channels": 1, "num_fmaps": 20, "fmap_inc_factor": 2, "downsample_factors": [list(factor)],
            "kernel_size_down": [K3, K3], "kernel_size_up": [K3], "outputs": {"3d_affs": {"dims": 6}}}


CASES = {   # name -> (pool factor, input shape, the POOL step is fused under the default rule)
    "mult4": ((1, 2, 2), (14, 20, 20), True),
    "overhang": ((1, 2, 2), (14, 22, 22), True),
    "factor3": ((1, 3, 3), (14, 28, 28), False),
    "factor222": ((2, 2, 2), (18, 20, 20), False),
}
_DEAD = (134, 139, 124, 137, -6, -11, -9)
_STOP = []


def _raw(shape):
    rng = np.random.default_rng(3)
    D, H, W = shape
    raw = rng.integers(0, 256, size=shape, dtype=np.uint8)
    blocks = rng.integers(0, 256, size=(D, -(-H // 4), -(-W // 4)), dtype=np.uint8).repeat(4, axis=1).repeat(4, axis=2)[:, :H, :W]
    raw[:, :, :W // 3] = 97
    raw[:, :, W // 3:2 * W // 3] = blocks[:, :, W // 3:2 * W // 3]
    return raw


def _child_main(name):
    import torch
    from bootstrapper_amd.unet import Model
    from bootstrapper_amd.synth import synthetic_state_dict
    factor, shape, _ = CASES[name]
    nc = _net(factor)
    m = Model(nc, precision="bf16x3").load_state_dict(synthetic_state_dict(nc, 2))
    m.profile(True)
    raw = torch.from_numpy(_raw(shape)).cuda()
    u8, f32 = m.predict_u8(raw, want_f32=True)
    torch.cuda.synchronize()
    totals = m.profile_totals()
    plan = m.plan_steps()
    hashes = {}
    pool_stats = None
    for p in plan:
        if p["type"] == "head" or not p["materialised"]:
            continue
        a = np.ascontiguousarray(m.debug_activation(p["step"]))
        hashes[str(p["step"])] = hashlib.sha1(a.tobytes()).hexdigest()
        hashes[f"{p['step']}lo"] = hashlib.sha1(np.ascontiguousarray(m.debug_activation(p["step"], 2)).tobytes()).hexdigest()
        if p["type"] == "pool":
            src = m.debug_activation(p["step"] - 1)
            f = factor
            D, H, W, C = src.shape
            win = src.reshape(D // f[0], f[0], H // f[1], f[1], W // f[2], f[2], C).transpose(0, 2, 4, 6, 1, 3, 5).reshape(-1, f[0] * f[1] * f[2])
            ties = int(((win == win.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
            zeros_all = int((win.max(axis=1) == 0).sum())
            zeros_some = int(((win == 0).any(axis=1) & (win.max(axis=1) > 0)).sum())
            pool_stats = {"windows": len(win), "ties": ties, "all_zero": zeros_all, "some_zero": zeros_some,
                          "equal_to_max_of_source": bool(np.array_equal(a, win.max(axis=1).reshape(a.shape)))}
    hashes["out_f32"] = hashlib.sha1(np.ascontiguousarray(f32[0].cpu().numpy()).tobytes()).hexdigest()
    hashes["out_u8"] = hashlib.sha1(np.ascontiguousarray(u8[0].cpu().numpy()).tobytes()).hexdigest()
    producer = [p for p in plan if p["type"] == "conv"][1]
    print("POOL-FUSE " + json.dumps({"hashes": hashes, "pool_launches": totals["pool"][2], "conv_launches": totals["conv"][2], "pool": pool_stats,
                                     "producer": producer["form"], "types": [p["type"] for p in plan], "materialised": [p["materialised"] for p in plan]}))


def _run(name, env):
    if _STOP:
        pytest.skip(f"a child process died earlier ({_STOP[0]}): no further GPU work in this run")
    base = {k: v for k, v in os.environ.items() if not k.startswith("BSMI_")}
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=dict(base, BSMI_WINO="2", **env), capture_output=True, text=True, timeout=120,
                           cwd=ROOT)
    except subprocess.TimeoutExpired:
        _STOP.append(f"{name} {env}: timeout")
        raise
    if r.returncode in _DEAD:
        _STOP.append(f"{name} {env}: exit status {r.returncode}")
    assert r.returncode == 0, f"{name} {env}:\n" + r.stdout[-4000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("POOL-FUSE ")][-1]
    return json.loads(line[len("POOL-FUSE "):])


@pytest.mark.parametrize("name", list(CASES))
def test_pooled_output_equals_the_separate_launch(name):
    fused_expected = CASES[name][2]
    new, old = _run(name, {}), _run(name, {"BSMI_POOL_FUSE": "0"})
    print(name, "default:", {k: new[k] for k in ("pool_launches", "pool", "producer")}, "| BSMI_POOL_FUSE=0:", {k: old[k] for k in ("pool_launches", "pool")})
    assert new["producer"] == "winograd F(4x4)" and old["producer"] == "winograd F(4x4)"
    assert new["types"].count("pool") == 1
    # the POOL step stays materialised either way
    assert all(m for t, m in zip(new["types"], new["materialised"]) if t == "pool")
    assert old["pool_launches"] == 1
    assert new["pool_launches"] == (0 if fused_expected else 1)
    assert new["conv_launches"] == old["conv_launches"]
    # the input does what the docstring says: ties, windows of zeros, windows with some zeros
    assert new["pool"]["ties"] > 0 and new["pool"]["all_zero"] > 0 and new["pool"]["some_zero"] > 0, new["pool"]
    assert new["pool"]["equal_to_max_of_source"] and old["pool"]["equal_to_max_of_source"]
    assert set(new["hashes"]) == set(old["hashes"])
    diff = [k for k in new["hashes"] if new["hashes"][k] != old["hashes"][k]]
    assert not diff, f"{name}: steps whose bits differ between the fused and the separate pool: {diff}"


if __name__ == "__main__":
    _child_main(sys.argv[1])
