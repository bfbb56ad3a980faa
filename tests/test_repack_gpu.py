"""Packing a handle's weights a second time, and destroying it (csrc/unet_pack.hip release(PackedConv / PackedWino / PackedH16),
used by bsmi_unet_finalize before a stage is packed again and by bsmi_unet_destroy).  Needs an MI355X.

Net A of tests/test_conv_below_up_gpu.py at its input (14, 52, 52), under BSMI_WINO=2 BSMI_H16=2 (read once per process: a
child process): two levels, 64 / 256 feature maps, a (1,2,2) decoder pass of two 3x3x3 stages.  Its decoder pass has every
device image a stage can have: the Winograd weights `w`, the residual branch whole (`res_w`) and cut by source (both
`res_part_w`), the first stage's `skip_w` and `below_w`, and, at 64 output channels, a halo-resident image beside every
gather image.

Steps: weights A into handle 1, finalise bf16x3, forward; weights B into the SAME handle, finalise again, forward; weights B
into a fresh handle 2, forward.  Handle 1's second outputs (float and u8) and every materialised activation must equal handle
2's bit for bit: an image left over from A, or one freed and still in use, would show there.  Both handles are then destroyed,
and A's outputs must differ from B's (the comparison would otherwise say nothing).  Values only."""
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


def _child_main():
    import torch
    from bootstrapper_amd._lib import check, lib
    from bootstrapper_amd.synth import synthetic_state_dict
    from bootstrapper_amd.unet import Model
    from test_conv_below_up_gpu import NETS
    nc, shape = NETS["A"][0], NETS["A"][1]
    sd_a, sd_b = synthetic_state_dict(nc, 5), synthetic_state_dict(nc, 6)
    x = torch.from_numpy(np.random.default_rng(11).integers(0, 256, size=shape, dtype=np.uint8)).cuda()

    def forward(m):
        u8, f32 = m.predict_u8(x, want_f32=True)
        torch.cuda.synchronize()
        plan = m.plan_steps()
        acts = [m.debug_activation(i) for i, p in enumerate(plan) if p["materialised"] and p["type"] != "head"]
        return u8[0].cpu().numpy(), f32[0].cpu().numpy(), acts, plan

    m1 = Model(nc, precision="bf16x3").load_state_dict(sd_a)
    u8_a, f32_a, _, plan = forward(m1)
    by = {(p["prefix"], p["conv"]): p for p in plan if p["type"] == "conv"}
    first, last = by[("unet.r_conv.0.0", 0)], by[("unet.r_conv.0.0", 1)]
    # the decoder pass takes the forms whose images the test is about
    assert first["form"] == "winograd F(4x4)" and first["below_up"] and "fused-up" in first["flags"], first
    assert last["form"] == "winograd F(4x4)" and "res-low" in last["flags"], last
    m1.load_state_dict(sd_b)          # the same handle: every stage is packed again
    u8_1, f32_1, acts_1, plan_1 = forward(m1)
    m2 = Model(nc, precision="bf16x3").load_state_dict(sd_b)
    u8_2, f32_2, acts_2, plan_2 = forward(m2)
    assert plan_1 == plan_2
    assert np.array_equal(f32_1.view(np.uint32), f32_2.view(np.uint32)) and np.array_equal(u8_1, u8_2)
    assert len(acts_1) == len(acts_2) and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(acts_1, acts_2))
    assert not np.array_equal(f32_a, f32_2)
    for m in (m1, m2):
        check(lib.bsmi_unet_destroy(m._h))
        m._h = None
    print(f"REPACK-OK {len(acts_1)} activations, float and u8 outputs bit-equal")


def test_repacked_handle_equals_a_fresh_one():
    env = dict({k: v for k, v in os.environ.items() if k not in ("BSMI_CONV_BELOW_UP", "BSMI_FUSE_UP_NARROW", "BSMI_FUSE_UP", "BSMI_WINO4")},
               BSMI_WINO="2", BSMI_H16="2")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "REPACK-OK" in r.stdout, r.stdout[-6000:] + r.stderr[-3000:]


if __name__ == "__main__":
    _child_main()
