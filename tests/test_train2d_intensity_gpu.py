"""`bs train` on the 2-D setups with `intensity` inside the `[augment2d]` table: SectionSource through the batched geometric
chain and then the batched intensity chain, on the store of tests/test_train2d_aug_gpu.py (input (48, 48), output (32, 32),
adj_slices 3 and once 1), and five Trainer steps of a small 2d_mtlsd net."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_train2d_aug_gpu import AFFS, INPUT, LSDS, OUTPUT, write_store  # noqa: E402

pytestmark = pytest.mark.gpu
OFF = {"noise_p": 0.0, "intensity_p": 0.0, "gamma_p": 0.0, "impulse_p": 0.0, "smooth_p": 0.0, "prob_missing": 0.0, "prob_low_contrast": 0.0}


def source(samples, augment, adj=3, seed=42):
    from bootstrapper_amd.augment2d import Aug2DParams
    from bootstrapper_amd.train import SectionSource
    params = Aug2DParams.from_config(augment) if isinstance(augment, dict) else augment
    return SectionSource(samples, INPUT, OUTPUT, adj, device=0, seed=seed, batch_size=10, lsds=LSDS, affs=AFFS, augment=params)


@pytest.fixture
def rounds(monkeypatch):
    """counts the rounds of _next_augmented (one coordinate launch each): [n]"""
    from bootstrapper_amd import augment2d as A
    n, real = [0], A.coords2d
    monkeypatch.setattr(A, "coords2d", lambda *a, **k: (n.__setitem__(0, n[0] + 1), real(*a, **k))[1])
    return n


def one_round_pairs(samples, table, adj, rounds):
    """yields (seed, geometric-only source, source with `table`, their first batches) for the seeds of 42 .. 51 at which both
    first batches took ONE round: the intensity draws follow a round's geometry, so only then do the two streams give one geometry"""
    for seed in range(42, 52):
        geo, other = source(samples, True, adj, seed), source(samples, table, adj, seed)
        rounds[0] = 0
        g, x = next(geo), next(other)
        if rounds[0] == 2:
            yield seed, geo, other, g, x


@pytest.mark.parametrize("adj", [3, 1])
def test_keys_shapes_dtypes_and_one_sequence_per_seed(tmp_path, adj):
    samples = write_store(tmp_path)
    geo, a, b = source(samples, True, adj), source(samples, {"intensity": True}, adj), source(samples, {"intensity": True}, adj)
    assert a.intensity.prob_missing == (0.05 if adj > 1 else 0.0) and geo.intensity is None
    g = next(geo)
    for _ in range(2):
        x, y = next(a), next(b)
        assert list(x) == list(g)
        for k in g:
            assert x[k].shape == g[k].shape and x[k].dtype == g[k].dtype and x[k].device == g[k].device and x[k].is_contiguous() == g[k].is_contiguous(), k
            assert bool(torch.isfinite(x[k]).all()), k
        assert all(torch.equal(x[k], y[k]) for k in x)                          # one seed, one sequence, bit for bit
        assert float(x["raw"].min()) >= -1.0 and float(x["raw"].max()) <= 1.0
    assert x["raw"].shape == (adj, 10) + INPUT
    assert a.rng.bit_generator.state == b.rng.bit_generator.state
    assert not torch.equal(next(source(samples, {"intensity": True}, adj))["raw"], g["raw"])    # the chain does change raw


def test_absent_or_all_zero_is_the_geometric_source(tmp_path):
    """`intensity` absent, false, or with every probability 0: the augment2d batches bit for bit, and the same generator state"""
    samples = write_store(tmp_path)
    geo = source(samples, True)
    others = [source(samples, {"intensity": False}), source(samples, {"intensity": OFF})]
    assert others[0].intensity is None and others[1].intensity is not None
    for _ in range(2):
        g = next(geo)
        for o in others:
            x = next(o)
            assert list(x) == list(g) and all(torch.equal(x[k], g[k]) for k in g)
    assert all(o.rng.bit_generator.state == geo.rng.bit_generator.state for o in others)


@pytest.mark.parametrize("adj", [3, 1])
def test_missing_sections_leave_labels_and_targets_alone(tmp_path, adj, rounds):
    """prob_missing = 1: every section of every draw is -1 or +1 throughout, and labels and targets are those of the
    geometric-only batch"""
    samples = write_store(tmp_path)
    seed, _, _, g, m = next(one_round_pairs(samples, {"intensity": dict(OFF, prob_missing=1.0)}, adj, rounds))
    flat = m["raw"].reshape(adj * 10, -1)
    assert bool(((flat == 1.0).all(dim=1) | (flat == -1.0).all(dim=1)).all())
    if adj == 3:
        assert bool((flat[:, 0] == 1.0).any()) and bool((flat[:, 0] == -1.0).any())         # thirty coins: both values occur
    assert [k for k in g if k != "raw"] and all(torch.equal(g[k], m[k]) for k in g if k != "raw")


def test_touched_and_untouched_draws_in_one_batch(tmp_path, rounds):
    """only low contrast, with probability 1/2 per section: a draw is untouched with probability 1/8, so most batches mix both
    kinds; the seed is the first at which the batch does.  The untouched draws' raw is the geometric-only batch's, bit for bit."""
    from bootstrapper_amd.augment import draw_intensity_plan
    samples = write_store(tmp_path)
    table = {"intensity": dict(OFF, prob_low_contrast=0.5)}
    touched = []
    for seed, geo, low, g, x in one_round_pairs(samples, table, 3, rounds):
        # the stream by hand: the geometry's draws are those the geometric source took, then ten plans in slot order
        rng = np.random.default_rng(0)
        rng.bit_generator.state = geo.rng.bit_generator.state
        plans = [draw_intensity_plan(rng, low.intensity, (3,) + INPUT) for _ in range(10)]
        assert rng.bit_generator.state == low.rng.bit_generator.state
        touched = [p.applied for p in plans]
        same = [bool(torch.equal(g["raw"][:, s], x["raw"][:, s])) for s in range(10)]
        print(f"seed {seed}: touched {touched}, raw equal to the geometric batch {same}")
        if any(touched) and not all(touched):
            break
    assert any(touched) and not all(touched), "both kinds of draw must occur"
    for s in range(10):
        if not touched[s]:
            assert same[s], f"slot {s}: an untouched draw differs from the geometric-only batch"
    assert not all(same[s] for s in range(10) if touched[s])                    # a low-contrast section is pulled towards its mean
    assert all(torch.equal(g[k], x[k]) for k in g if k != "raw")


def test_five_trainer_steps_with_augment2d_intensity(tmp_path):
    """`bs train` on the small 2d_mtlsd net of tests/test_train2d_aug_gpu.py with `[augment2d] intensity = true`"""
    from bootstrapper_amd.train import run_training
    samples = write_store(tmp_path)
    setup = tmp_path / "setup_01"
    setup.mkdir()
    nc = {"in_channels": 1, "adj_slices": 3, "num_fmaps": 4, "fmap_inc_factor": 2, "downsample_factors": [[2, 2], [2, 2], [2, 2]],
          "kernel_size_down": [[[3, 3], [3, 3]]] * 4, "kernel_size_up": [[[3, 3], [3, 3]]] * 3,
          "input_shape": [108, 108], "output_shape": [16, 16], "inputs": {"raw": {"dims": 1}},
          "outputs": {"2d_lsds": {"dims": 6, "sigma": 80, "downsample": 2},
                      "2d_affs": {"dims": 2, "neighborhood": [[-1, 0], [0, -1]], "grow_boundary": 1}}}
    (setup / "net_config.json").write_text(json.dumps(nc))
    cfg = tmp_path / "train.toml"
    cfg.write_text(f'setup_dir = "{setup}"\nvoxel_size = [40, 4, 4]\nmax_iterations = 5\n'
                   f'[[samples]]\nraw = "{samples[0]["raw"]}"\nlabels = "{samples[0]["labels"]}"\n[augment2d]\nintensity = true\n')
    logs = []
    assert run_training(str(cfg), log=logs.append) == 5
    losses = [float(l.split("train_loss")[1]) for l in logs if "train_loss" in l]
    assert len(losses) >= 1 and all(np.isfinite(losses)), logs
    assert any("augment2d.intensity" in l and "Clahe" in l for l in logs)
