"""The F(4x4) input transforms (csrc/wino.hip: wino4_in_kernel, wino4_in_up_kernel) give a thread a SEGMENT of S tiles of a
tile row; S is 1 by the rule, or set by BSMI_WINO_IN_SEG (0 = whole rows, the decomposition before segments existed;
n > 0 = S = min(n, Tx)).  The arithmetic of a tile does not depend on S, so the forward pass is the same BIT FOR BIT under
every setting: a child process per setting (the switch is read once per process) prints SHA-256 hashes of the f32 output of
the forward pass and of predict_u8, and they must equal those of BSMI_WINO_IN_SEG=0.  Needs an MI355X.

Net: three levels of the shipped family (12 / 60 / 300 channels, factors (1, 2, 2), 3x3x3 kernels, synthetic weights), split-bf16,
BSMI_WINO=2 BSMI_WINO4=2: every 3x3x3 stage in the F(4x4) form, the fused-upsampling transform included (the plan printed
by BSMI_PLAN_DEBUG must name F(4x4) on at least eight distinct stages, or the comparison would be vacuous).
Inputs (24, 100, 100) and (24, 100, 84): stage outputs 98/96, 46/44, 20/18, 34/32, 62/60 in the plane of the first, i.e.
Tx in {25, 24, 12, 11, 5, 5, 9, 8, 16, 15} -- overhanging and exact last tiles, Tx = 0, 1, 2 mod 3, sources of 12, 60 and 300
channels (4, 16 and 76 channel groups per tile: the last straddles a wave), two-source stages (skip + upsampled); the second
shape has Ty != Tx (the planner takes both shapes as they are: ten F(4x4) stages each).  S in {rule, 1, 2, 3, 64}: 64 exceeds
every Tx (one segment per row, reached through the n > 0 branch of the launcher).
The whole-row run is tied to something that is itself checked: within the suite's split-bf16 tolerance of oracle/unet_ref.py.
"""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

NET = {"in_channels": 1, "num_fmaps": 12, "fmap_inc_factor": 5, "downsample_factors": [[1, 2, 2], [1, 2, 2]],
       "kernel_size_down": [[[3, 3, 3], [3, 3, 3]]] * 3, "kernel_size_up": [[[3, 3, 3], [3, 3, 3]]] * 2, "outputs": {"3d_affs": {"dims": 6}}}
SHAPES = [(24, 100, 100), (24, 100, 84)]
ENV = {"BSMI_WINO": "2", "BSMI_WINO4": "2", "BSMI_PLAN_DEBUG": "1"}
_DEAD = (134, 139, 124, 137, -6, -11, -9)
_STOP = []            # a child ended on a signal or a timeout: no further GPU work in this run


def _case(shape):
    from bootstrapper_amd.synth import synthetic_state_dict
    raw = np.random.default_rng(7).integers(0, 256, size=shape, dtype=np.uint8)
    return synthetic_state_dict(NET, 3), raw


def _run_child(seg, dump=None):
    """-> {shape: (sha of the f32 forward, sha of predict_u8)}, number of distinct stages the plan names F(4x4) on"""
    if _STOP:
        pytest.skip(f"a child process died earlier ({_STOP[0]}): no further GPU work in this run")
    env = dict(os.environ, **ENV)
    env.pop("BSMI_WINO_IN_SEG", None)
    if seg is not None:
        env["BSMI_WINO_IN_SEG"] = str(seg)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), dump or "-"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _STOP.append(f"BSMI_WINO_IN_SEG={seg}: timeout")
        raise
    if r.returncode in _DEAD:
        _STOP.append(f"BSMI_WINO_IN_SEG={seg}: exit status {r.returncode}")
    assert r.returncode == 0, f"BSMI_WINO_IN_SEG={seg}:\n" + r.stdout[-3000:] + r.stderr[-3000:]
    hashes = {}
    for line in r.stdout.splitlines():
        if line.startswith("SEG-HASH "):
            _, shape, f32, u8 = line.split()
            hashes[shape] = (f32, u8)
    stages = set(re.findall(r"\[bsmi plan\] (\S+ conv \d+): out \S+ .*winograd F\(4x4,3x3\)", r.stderr + r.stdout))
    return hashes, len(stages)


@pytest.fixture(scope="module")
def whole_rows(tmp_path_factory):
    """BSMI_WINO_IN_SEG=0: the hashes every other setting has to reproduce, and the f32 outputs for the oracle"""
    dump = str(tmp_path_factory.mktemp("wino_in_seg") / "whole_rows.npz")
    hashes, stages = _run_child(0, dump)
    return hashes, stages, np.load(dump)


def test_whole_rows_run_matches_the_oracle(whole_rows):
    from oracle import unet_ref as R
    from test_unet_gpu import TOL_BF16X3
    hashes, stages, outs = whole_rows
    assert stages >= 8, stages
    assert sorted(hashes) == sorted("x".join(map(str, s)) for s in SHAPES)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cfg = {k: v for k, v in NET.items() if k != "outputs"}
    for shape in SHAPES:
        sd, raw = _case(shape)
        ref = R.predict_block(cfg, sd, raw, ["affs_head"])[0]
        got = outs["x".join(map(str, shape))]
        assert got.shape == ref.shape
        err = float(np.abs(got - ref).max())
        print(f"{shape} whole rows: max abs err vs oracle {err:.3e}")
        assert err < TOL_BF16X3


@pytest.mark.parametrize("seg", [None, 1, 2, 3, 64], ids=lambda s: "rule" if s is None else f"S={s}")
def test_segments_reproduce_whole_rows_bit_for_bit(whole_rows, seg):
    ref_hashes, _, _ = whole_rows
    hashes, stages = _run_child(seg)
    print(seg, hashes, stages)
    assert stages >= 8, stages
    assert hashes == ref_hashes


# ---- child process ----------------------------------------------------------------------------------------------------------
def _main(dump):
    from bootstrapper_amd.unet import Model
    keep = {}
    m = None
    for shape in SHAPES:
        sd, raw = _case(shape)
        if m is None:
            m = Model(NET, device=0, precision="bf16x3").load_state_dict(sd)
        u8, f32 = m.predict_u8(torch.from_numpy(raw).cuda(0), want_f32=True)
        f = f32[0].cpu().numpy()
        u = u8[0].cpu().numpy()
        name = "x".join(map(str, shape))
        print(f"SEG-HASH {name} {hashlib.sha256(np.ascontiguousarray(f).tobytes()).hexdigest()} "
              f"{hashlib.sha256(np.ascontiguousarray(u).tobytes()).hexdigest()}")
        keep[name] = f
    if dump != "-":
        np.savez(dump, **keep)


if __name__ == "__main__":
    _main(sys.argv[1])
