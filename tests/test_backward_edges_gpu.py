"""Case E of the per-launch parity of the training backward pass (tests/test_backward_gpu.py holds cases A - D): the walk of that file,
unchanged, on the nets of tests/edge_nets.py whose channel counts sit on the tile edges of the weight-gradient and input-gradient
launchers.  Needs an MI355X.

E1, E3, E4, E6, E9, E10 and E13 in f32 and in split-bf16 arithmetic, one deterministic split-bf16 run each of E3 and E6; every
element, weight gradients unsampled; gates from the reference alone (tests/bwd_ref.py).  The last test holds what
Trainer.backward_steps() reports to the edges the nets exist for, written out by hand:

  weight gradient   N = 32 and N = 64 exactly (the 32- and 64-row tiles full), N = 65 (the 128-row tile with one row over 64), the
                    128-row tile with several N blocks (N > 128); C = 64 exactly, C = 65 (a second 64-channel C-tile holding one
                    real channel)
  input gradient    N = the concatenated input channels of the stage: BN 160, BN 256 in one tile, BN 320 filled exactly, 2 x 256

The first run of this file found that the head backward kernel took at most 32 input channels (the forward's head takes 64) and
refused E6, E9, E10 and E13 in the middle of a step: head_bwd_kernel<true> (csrc/train_bwd.hip) serves 33 to 64 channels since.

Largest err / S per arithmetic and form over case E on the MI355X with the largest gate of those launches (records, not gates;
the BACKWARD-FORM lines, the deterministic runs folded into their arithmetic; also in DESIGN.md section 2, "Case E"):

  arithmetic   form                                       largest err / S      largest g_acc
  f32          input gradient f32 (/ split-K)             1.25e-05 / 2.16e-06  3.79e-05 / 2.26e-05
  f32          weight gradient wave-f32 KX 1 / KX 3       5.88e-06 / 9.44e-06  7.50e-05 / 9.38e-05
  f32          weight gradient tiled-f32 KX 1 / KX 3      3.83e-06 / 7.00e-06  5.34e-05 / 6.28e-05
  f32          bias sums, head weights                    1.28e-05, 1.29e-06   1.20e-04, 3.30e-05
  split-bf16   input gradient split-bf16 raw (/ split-K)  2.16e-05 / 2.12e-05  8.18e-05 / 8.18e-05
  split-bf16   training forward, fused split launch       3.89e-05             8.01e-05
  split-bf16   weight gradient split-bf16 KX 1, six tiles 1.38e-05 .. 2.60e-05 7.69e-05
  split-bf16   weight gradient split-bf16 KX 3, six tiles 1.73e-05 .. 2.92e-05 8.59e-05
  split-bf16   bias sums fused / colsum, head weights     1.72e-05 / 1.98e-06, 1.33e-06   1.65e-04 / 1.39e-04, 2.91e-05
  both         upsampling backward scatter / gather, err / bound   0.30 / 0.26   1
Wall time of this file on the MI355X: 39 s (17 tests; E13 in split-bf16 7.8 s, in f32 4.1 s, every other test 3.1 s or less).
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import edge_nets as E  # noqa: E402
import layer_ref as L  # noqa: E402
import test_backward_gpu as TB  # noqa: E402

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, os.cpu_count() or 1))

RECORD = TB.Record()
WGRAD = {}     # arithmetic -> {(family, N, C, tile)} of the weight-gradient launches met
DGRAD = {}     # arithmetic -> {(BN, N-tiles, exact fit, N)} of the input-gradient launches met


def run_edge(tag, arith):
    nc, sd, _ = E.edge_case(tag)
    shape = E.shape_of(tag)
    facts = TB.run_case(f"E:{tag}", nc, sd, shape, arith, record=RECORD)
    ops = L.walk(nc, shape)
    a = arith.split("+")[0]
    for o, b in zip(ops, facts["bsteps"]):
        if b["type"] != "conv":
            continue
        for w in b["wgrad"]:
            WGRAD.setdefault(a, set()).add((w["family"], w["n"], w["c"], tuple(w["tile"])))
        d = b["dgrad"]
        if d:
            n = sum(c for _, _, c in o["src"])
            DGRAD.setdefault(a, set()).add((d["bn"], -(-n // d["bn"]), n % d["bn"] == 0, n))
    return facts


@pytest.mark.parametrize("arith", ["f32", "split-bf16"])
@pytest.mark.parametrize("tag", E.BACKWARD_TAGS)
def test_case_e_edge_nets(tag, arith):
    run_edge(tag, arith)


@pytest.mark.parametrize("tag", ["E3", "E6"])
def test_case_e_deterministic(tag):
    facts = run_edge(tag, "split-bf16+deterministic")
    assert any(w["det_workspace"] for b in facts["bsteps"] if b["type"] == "conv" for w in b["wgrad"])


def test_every_gradient_tile_edge_was_reached():
    """(last in the module: it needs the tests above to have run)"""
    for line in RECORD.lines():
        print(line)
    for a in sorted(WGRAD):
        print(f"EDGE-WGRAD {a}: {sorted(WGRAD[a])}")
        print(f"EDGE-DGRAD {a}: {sorted(DGRAD[a])}")
    sp = WGRAD["split-bf16"]
    split = {(n, c, t) for fam, n, c, t in sp if fam == "split-bf16"}
    # N edges: the tile is the launcher's, the count is the net's
    assert any(n == 32 and t[0] == 32 for n, c, t in split), "no split-bf16 weight gradient with N = 32 on the 32-row tile"
    assert any(n == 64 and t[0] == 64 for n, c, t in split), "no split-bf16 weight gradient with N = 64 on the 64-row tile"
    assert any(n == 65 and t[0] == 128 for n, c, t in split), "no split-bf16 weight gradient with N = 65 on the 128-row tile"
    assert any(n > 128 and t[0] == 128 for n, c, t in split), "no split-bf16 weight gradient with several blocks of the 128-row tile"
    assert any(n == 128 * 5 and t[0] == 128 for n, c, t in split), "no split-bf16 weight gradient that fills its 128-row blocks (N = 640)"
    # C edges
    assert any(c == 64 and t[1] == 64 for n, c, t in split), "no split-bf16 weight gradient with C = 64 on the 64-channel tile"
    assert any(c == 65 and t[1] == 64 for n, c, t in split), "no split-bf16 weight gradient with C = 65: a second C-tile with one real channel"
    # ... and the f32 families saw the same counts
    f32 = {(n, c) for fam, n, c, t in WGRAD["f32"]}
    assert {(32, 32), (64, 64), (65, 65), (160, 160), (640, 640)} <= f32, sorted(f32)
    # input gradients: N = the stage's concatenated input channels
    for a in ("f32", "split-bf16"):
        d = DGRAD[a]
        assert any(bn == 160 and nt == 1 for bn, nt, ex, n in d), (a, "no input gradient on the 160-column tile", sorted(d))
        assert any(bn == 256 and nt == 1 for bn, nt, ex, n in d), (a, "no input gradient on a single 256-column tile", sorted(d))
        assert (320, 1, True, 320) in d, (a, "no input gradient that fills the 320-column tile exactly", sorted(d))
        assert (256, 2, False, 384) in d, (a, "no input gradient on 2 x 256 columns with a half-full last tile", sorted(d))
