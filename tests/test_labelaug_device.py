"""`label_augment` of `bs train` on the device: augment_labels.warp_labels against the rule "labels are 0 outside the block"
evaluated in numpy on the device's own read-back coordinates (tests/labelaug_ref.py; exact, no voxel left out), plans whose result
needs no reference, the refusals, the order of the nodes and the random streams of train.SyntheticSource, bit-equality of the
batches with and without the key, and a short run.  The small configs are those of tests/test_train_synth_gpu.py."""
import json
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_ref as R  # noqa: E402
import labelaug_ref as L  # noqa: E402
from bootstrapper_amd import augment as A  # noqa: E402
from bootstrapper_amd import augment_labels as AL  # noqa: E402

pytestmark = pytest.mark.gpu

NET = {"num_fmaps": 3, "num_fmaps_out": 5, "fmap_inc_factor": 2, "downsample_factors": [[1, 2, 2]] * 3,
       "kernel_size_down": [[[1, 3, 3], [1, 3, 3]]] * 2 + [[[3, 3, 3], [3, 3, 3]]] * 2, "kernel_size_up": [[[3, 3, 3], [3, 3, 3]]] * 3}
OUT = {"3d_affs": {"dims": 9, "neighborhood": [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -9, 0], [0, 0, -9], [-3, 0, 0], [0, -27, 0], [0, 0, -27]],
                   "grow_boundary": 1}}
CONFIGS = {
    "from_2d_mtlsd": dict(NET, input_shape=[21, 100, 100], output_shape=[1, 8, 8], outputs=OUT,
                          inputs={"2d_lsds": {"dims": 6, "sigma": 10, "downsample": 2, "grow_boundary": 1},
                                  "2d_affs": {"dims": 6, "neighborhood": [[-1, 0], [0, -1], [-9, 0], [0, -9], [-27, 0], [0, -27]], "grow_boundary": 1}}),
    "from_3d_lsd": dict(NET, input_shape=[22, 100, 100], output_shape=[2, 8, 8], outputs=OUT,
                        inputs={"3d_lsds": {"dims": 10, "sigma": 10, "downsample": 2, "grow_boundary": 1}}),
}
VS = (40, 4, 4)
CFG = {"voxel_size": list(VS), "synthetic_labels": True}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda(0)


def warp(lab, plan):
    return AL.warp_labels(dev(lab), plan).cpu().numpy()


# ---- warp_labels on its own inputs ----

@pytest.mark.parametrize("block", sorted(R.BLOCKS))
@pytest.mark.parametrize("spacing", sorted(R.SPACINGS))
def test_warp_labels_is_the_rule_on_the_device_s_coordinates(block, spacing):
    shape = R.BLOCKS[block]
    plan = R.build_plan(shape, R.SPACINGS[spacing], seed=11)
    lab = R.build_crops(shape, seed=12)[1]
    coords = A.coords(plan, L.BOX_LO, 0).cpu().numpy()          # the planes warp_labels makes for itself: same plan, same launch
    want = L.rule(coords, lab)
    got = AL.warp_labels(dev(lab), plan)
    assert got.dtype == torch.int64 and tuple(got.shape) == shape and got.is_contiguous()
    got = got.cpu().numpy()
    share = float((want == 0).mean())
    print(f"{block} {spacing}: {100 * share:.1f} % of the voxels lie outside the block")
    assert 0.0 < share < 1.0                                    # both branches of the rule
    assert np.array_equal(got, want)                            # exact, every voxel
    assert set(np.unique(got)) <= set(np.unique(lab)) | {0}     # a read outside the padded block would show
    assert not np.array_equal(L.clamping(coords, lab), want)


@pytest.fixture(scope="module")
def labels():
    return R.build_crops((5, 24, 24), seed=3)[1]


def test_identity_plan_returns_the_labels_without_a_launch(labels, monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("an identity plan launches nothing")
    monkeypatch.setattr(A, "coords", no_launch)
    monkeypatch.setattr(A, "sample_labels", no_launch)
    x = dev(labels)
    out = AL.warp_labels(x, A.AugPlan((5, 24, 24)))
    assert out is x and np.array_equal(out.cpu().numpy(), labels)


@pytest.mark.parametrize("mirror", [(True, False, False), (False, True, False), (False, False, True), (True, True, True)])
def test_mirror_only_plans_are_flips(labels, mirror):
    flip = tuple(slice(None, None, -1) if f else slice(None) for f in mirror)
    assert np.array_equal(warp(labels, A.AugPlan((5, 24, 24), mirror=mirror)), labels[flip])


def test_swap_only_plan_is_a_transpose(labels):
    assert np.array_equal(warp(labels, A.AugPlan((5, 24, 24), swap=True)), labels.transpose(0, 2, 1))


def test_shift_only_plan_lets_zeros_in(labels):
    shifts = np.array([[0, 3, -8, 8, 1], [-7, 0, 8, -2, -30]], dtype=np.int32)
    got = warp(labels, A.AugPlan((5, 24, 24), shifts=shifts))
    assert np.array_equal(got, L.shifted_expected(labels, shifts))
    assert (got[4] == 0).all() and (got[2, :8] == 0).all() and (got[2, :, -8:] == 0).all() and (got[0, :, :7] == 0).all() and (got[0, :, 7:] != 0).all()


@pytest.mark.parametrize("shape", [(5, 24, 24), (3, 17, 33)])
def test_scaling_lets_a_frame_of_zeros_in(shape):
    lab = R.build_crops(shape, seed=4)[1]
    plan = L.mild_plan(shape)
    coords = A.coords(plan, L.BOX_LO, 0).cpu().numpy()
    want = L.rule(coords, lab)
    got = warp(lab, plan)
    assert np.array_equal(got, want)                            # the zero voxels are exactly those the rule names
    zero = got == 0
    per = [zero.all(axis=tuple(b for b in range(3) if b != a)) for a in range(3)]
    assert np.array_equal(zero, per[0][:, None, None] | per[1][None, :, None] | per[2][None, None, :])   # a frame
    for a, n in enumerate(shape):
        c = (n - 1) / 2.0
        t = np.abs(np.arange(n) - c) * 1.2
        assert per[a][t > c + 0.75].all() and not per[a][t < c + 0.25].any(), a
    assert 0.0 < zero.mean() < 1.0


def test_refusals(labels):
    plan = A.AugPlan((5, 24, 24), mirror=(True, False, False))
    x = dev(labels)
    with pytest.raises(ValueError, match="int64 CUDA"):
        AL.warp_labels(x.to(torch.int32), plan)
    with pytest.raises(ValueError, match="int64 CUDA"):
        AL.warp_labels(x.cpu(), plan)
    with pytest.raises(ValueError, match="int64 CUDA"):
        AL.warp_labels(x[None], plan)
    with pytest.raises(ValueError, match="contiguous"):
        AL.warp_labels(x.transpose(1, 2), plan)                 # the right shape, the wrong strides
    with pytest.raises(ValueError, match=r"shape \(5, 24, 24\) for a plan of \(5, 24, 25\)"):
        AL.warp_labels(x, A.AugPlan((5, 24, 25)))
    torch.cuda.synchronize()


# ---- the source ----

@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_order_and_streams(name):
    """labels() is create_labels -> the plan from (seed, 2) -> warp_labels -> grow_boundary -> obfuscate, replayed by hand"""
    from bootstrapper_amd import synth_labels as S
    from bootstrapper_amd.train import SyntheticSource
    nc = CONFIGS[name]
    inp = tuple(nc["input_shape"])
    src = SyntheticSource(nc, VS, 0, seed=42, label_augment=True)
    hand = SyntheticSource(nc, VS, 0, seed=42, label_augment=True)      # lends its engine; its streams are not used
    eng = hand._engine()
    rng, lrng = random.Random(42), np.random.default_rng((42, 2))
    params = AL.LabelAugParams().to_aug_params(VS)
    changed = False
    for _ in range(2):
        got_lab, got_obf = src.labels()
        made = eng.create_labels(S.draw_plan(rng, inp, hand.aniso))
        lab = AL.warp_labels(made, A.draw_plan(lrng, params, inp, VS))
        changed = changed or not torch.equal(lab, made)
        lab = eng.grow_boundary(lab, rng.getrandbits(64), hand.in_grow)
        obf = eng.obfuscate(lab, rng)
        assert got_lab.dtype == torch.int64 and tuple(got_lab.shape) == inp
        assert torch.equal(got_lab, lab) and torch.equal(got_obf, obf)
    assert changed
    assert src.rng.getstate() == rng.getstate() and src.label_rng.random() == lrng.random()


@pytest.fixture(scope="module")
def batches():
    """three batches of each config: of a source constructed as before this key existed, and of the source with the key; made once"""
    from bootstrapper_amd.train import SyntheticSource, make_sample_source
    out = {}
    for name, nc in CONFIGS.items():
        plain = SyntheticSource(nc, VS, device=0, seed=42)
        keyed = make_sample_source(dict(CFG, label_augment=True), nc, 0, 0)
        out[name] = ([next(plain) for _ in range(3)], [next(keyed) for _ in range(3)], plain.rng.getstate())
    return out


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_without_the_key_the_batches_are_the_plain_ones(batches, name):
    from bootstrapper_amd.train import make_sample_source
    plain, _, state = batches[name]
    for cfg in (CFG, dict(CFG, label_augment=False)):
        src = make_sample_source(cfg, CONFIGS[name], 0, 0)
        assert src.label_augment is None and src.label_rng is None
        for want in plain:
            got = next(src)
            assert list(got) == list(want)
            for k in want:
                assert torch.equal(got[k], want[k]), k
        assert src.rng.getstate() == state


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_batches_with_the_key(batches, name):
    from bootstrapper_amd.train import make_sample_source
    nc = CONFIGS[name]
    plain, keyed, _ = batches[name]
    again = make_sample_source(dict(CFG, label_augment=True), nc, 0, 0)
    beside = make_sample_source(dict(CFG, label_augment=True, input_augment=True), nc, 0, 0)
    differs = False
    for want, old in zip(keyed, plain):
        got, both = next(again), next(beside)
        assert list(got) == list(want) == list(both) == ["raw", "gt_affs", "affs_weights"]
        for k in want:
            assert want[k].shape == old[k].shape and want[k].dtype == old[k].dtype and want[k].is_contiguous(), k
            assert torch.equal(got[k], want[k]), k               # one seed, one sequence of batches, bit for bit
        # the input augmentation beside it does not touch the labels' streams: the targets are those of label_augment alone
        assert torch.equal(both["gt_affs"], want["gt_affs"]) and torch.equal(both["affs_weights"], want["affs_weights"])
        assert bool(torch.isfinite(want["raw"]).all()) and float(want["raw"].min()) >= 0.0 and float(want["raw"].max()) <= 1.0
        assert bool(((want["gt_affs"] == 0) | (want["gt_affs"] == 1)).all()) and bool(torch.isfinite(want["affs_weights"]).all())
        differs = differs or not torch.equal(want["raw"], old["raw"])
    assert differs


def run(tmp_path, extra):
    from bootstrapper_amd.train import latest_checkpoint, run_training
    setup = tmp_path / "setup_01"
    setup.mkdir()
    (setup / "net_config.json").write_text(json.dumps(CONFIGS["from_2d_mtlsd"]))
    cfg = tmp_path / "train.toml"
    cfg.write_text(f'setup_dir = "{setup}"\nvoxel_size = [40, 4, 4]\nmax_iterations = 3\nsave_checkpoints_every = 3\nsave_snapshots_every = 1000\n'
                   'synthetic_labels = true\n' + extra)
    logs = []
    assert run_training(str(cfg), log=logs.append) == 3
    assert latest_checkpoint(str(setup))[1] == 3
    losses = [float(l.split("train_loss")[1].split()[0].strip("=:, ")) for l in logs if "train_loss" in l]
    assert losses and all(math.isfinite(v) for v in losses)
    return [l for l in logs if l.startswith("note: synthetic labels")]


def test_run_training_with_label_augment(tmp_path):
    from bootstrapper_amd.train import SyntheticSource
    note = run(tmp_path, "label_augment = true\n")
    assert len(note) == 1 and "`label_augment`" in note[0] and "SimpleAugment" not in note[0] and "DeformAugment" not in note[0]
    assert note[0].split("not built: ")[1].startswith(SyntheticSource.NOT_BUILT_WITH_LABEL_AUGMENT)


def test_run_training_with_both_keys_and_without(tmp_path):
    from bootstrapper_amd.train import SyntheticSource
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    note = run(tmp_path / "a", "label_augment = true\ninput_augment = true\n")
    assert len(note) == 1 and "`label_augment`" in note[0] and "`input_augment`" in note[0] and "SimpleAugment" not in note[0]
    assert note[0].endswith("not built: " + SyntheticSource.NOT_BUILT_WITH_BOTH)
    # the line logged without the key is the one logged before it existed
    assert run(tmp_path / "b", "") == [f"note: synthetic labels (synthetic_labels = true); not built: {SyntheticSource.NOT_BUILT}"]
