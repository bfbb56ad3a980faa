"""`input_augment` of `bs train` on the second-stage setups: the batches of SyntheticSource with the input augmentation against
the plain source's, and a short run.  The small configs are those of tests/test_train_synth_gpu.py."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augin_ref as R  # noqa: E402

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
CFG = {"voxel_size": [40, 4, 4], "synthetic_labels": True}
OFF = {"noise_p": 0, "channel_intensity_p": 0, "section_intensity_p": 0, "smooth_p": 0, "prob_low_contrast": 0}


@pytest.fixture(scope="module")
def plain():
    """the first three batches of the un-augmented source of each config, and the state its stream is left in; made once"""
    from bootstrapper_amd.train import make_sample_source
    out = {}
    for name, nc in CONFIGS.items():
        src = make_sample_source(CFG, nc, 0, 0)
        out[name] = ([next(src) for _ in range(3)], src.rng.getstate())
    return out


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_without_the_key_and_with_every_node_off_the_batches_are_the_plain_ones(plain, name):
    from bootstrapper_amd.train import make_sample_source
    batches, state = plain[name]
    for cfg in (dict(CFG, input_augment=False), dict(CFG, input_augment=OFF)):
        src = make_sample_source(cfg, CONFIGS[name], 0, 0)
        for want in batches:
            got = next(src)
            assert list(got) == list(want)
            for k in want:
                assert torch.equal(got[k], want[k]), k
        assert src.rng.getstate() == state                        # the plain stream is where the plain source left it


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_batches_with_the_key(plain, name):
    from bootstrapper_amd.train import make_sample_source
    nc = CONFIGS[name]
    batches, state = plain[name]
    a, b = (make_sample_source(dict(CFG, input_augment=True), nc, 0, 0) for _ in range(2))
    differs = False
    for want in batches:
        got, again = next(a), next(b)
        assert list(got) == list(want) == ["raw", "gt_affs", "affs_weights"]
        for k in want:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and got[k].is_contiguous(), k
            assert torch.equal(got[k], again[k]), k               # one seed, one sequence of batches, bit for bit
        assert torch.equal(got["gt_affs"], want["gt_affs"]) and torch.equal(got["affs_weights"], want["affs_weights"])
        assert bool(torch.isfinite(got["raw"]).all()) and float(got["raw"].min()) >= 0.0 and float(got["raw"].max()) <= 1.0
        differs = differs or not torch.equal(got["raw"], want["raw"])
    assert differs                                                # some node of some plan is applied within three batches
    assert a.rng.getstate() == state


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_low_contrast_alone_against_the_plain_batch(plain, name):
    """prob_low_contrast = 1, everything else 0: every section of every input array is pulled towards its mean over (C, H, W)"""
    from bootstrapper_amd import augment_inputs as A
    from bootstrapper_amd.train import make_sample_source
    want = plain[name][0][0]
    src = make_sample_source(dict(CFG, input_augment=dict(OFF, prob_low_contrast=1)), CONFIGS[name], 0, 0)
    got = next(src)
    assert torch.equal(got["gt_affs"], want["gt_affs"]) and torch.equal(got["affs_weights"], want["affs_weights"])
    assert sum(hi - lo for _, lo, hi in src.arrays) == want["raw"].shape[1]
    for key, lo, hi in src.arrays:
        x = want["raw"][0, lo:hi].contiguous()
        m = A.group_mean(x, 1).cpu().numpy().astype(np.float64)[None, :, None, None]     # the means the node read, as the device takes them
        diff, ratio = R.worst(got["raw"][0, lo:hi].cpu().numpy(), m + (x.cpu().numpy().astype(np.float64) - m) * 0.1, R.contrast_gate(0.1))
        print(f"{name} {key}: largest |raw - (m + (plain - m) 0.1)| {diff:.3e}, {ratio:.3f} of its gate")
        assert ratio <= 1.0, (key, diff, ratio)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_run_training_with_input_augment(tmp_path, name):
    from bootstrapper_amd.train import latest_checkpoint, run_training
    setup = tmp_path / "setup_01"
    setup.mkdir()
    (setup / "net_config.json").write_text(json.dumps(CONFIGS[name]))
    cfg = tmp_path / "train.toml"
    cfg.write_text(f'setup_dir = "{setup}"\nvoxel_size = [40, 4, 4]\nmax_iterations = 3\nsave_checkpoints_every = 3\nsave_snapshots_every = 1000\n'
                   'synthetic_labels = true\ninput_augment = true\n')
    logs = []
    assert run_training(str(cfg), log=logs.append) == 3
    ckpt, step = latest_checkpoint(str(setup))
    assert step == 3 and os.path.basename(ckpt) == "model_checkpoint_3.ckpt"
    losses = [float(l.split("train_loss")[1].split()[0].strip("=:, ")) for l in logs if "train_loss" in l]
    assert losses and all(math.isfinite(v) for v in losses)
    note = [l for l in logs if "input_augment" in l]
    assert note and "SmoothAugment" in note[0] and "not built" in note[0] and "DeformAugment" in note[0].split("not built")[1]
    assert "NoiseAugment" not in note[0].split("not built")[1]


def test_input_augment_on_a_first_stage_net_raises():
    from bootstrapper_amd.train import make_sample_source
    first = {"input_shape": [8, 32, 32], "output_shape": [4, 16, 16],
             "outputs": {"3d_affs": {"dims": 3, "neighborhood": [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]}}}
    with pytest.raises(NotImplementedError, match=r"input_augment: not built for the 3d_affs setup.*`augment`"):
        make_sample_source({"samples": [], "input_augment": True}, first, 0, 0)
