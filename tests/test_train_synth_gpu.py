"""`bs train` on the second-stage setups with `synthetic_labels = true`: the batches of SyntheticSource and a short run.
Small nets with the channel counts of the from_2d_mtlsd_f3i2 golden at the smallest input the net takes ((21, 100, 100) ->
(1, 8, 8); the 3-D descriptors want every axis a multiple of their downsample factor, hence 22 -> 2 there)."""
import json
import math
import os

import pytest
import torch

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


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_batches(name):
    from bootstrapper_amd.train import make_sample_source
    nc = CONFIGS[name]
    a, b, c = (make_sample_source(CFG, nc, 0, rank) for rank in (0, 0, 1))
    first = [next(a), next(a), next(a)]
    again = [next(b), next(b), next(b)]
    other = next(c)
    channels = sum(v["dims"] for v in nc["inputs"].values())
    differs = False
    for x, y in zip(first, again):
        assert list(x) == ["raw", "gt_affs", "affs_weights"]
        assert tuple(x["raw"].shape) == (1, channels, *nc["input_shape"]) and x["raw"].dtype == torch.float32 and x["raw"].is_contiguous()
        assert tuple(x["gt_affs"].shape) == tuple(x["affs_weights"].shape) == (9, *nc["output_shape"])
        for k in x:
            assert torch.equal(x[k], y[k]), k                     # one seed, one sequence of batches, bit for bit
        assert bool(torch.isfinite(x["raw"]).all()) and float(x["raw"].min()) >= 0.0 and float(x["raw"].max()) <= 1.0
        assert float(x["raw"].max()) > 0.0
        assert bool(((x["gt_affs"] == 0) | (x["gt_affs"] == 1)).all())
        assert bool(torch.isfinite(x["affs_weights"]).all()) and float(x["affs_weights"].min()) >= 0.0
        differs = differs or not torch.equal(x["raw"], other["raw"])
    assert differs                                                # seed 42 + rank
    assert not torch.equal(first[0]["raw"], first[1]["raw"])


def test_labels_of_the_source():
    """the labels behind a batch: input_shape, int64, obfuscation changes some voxels over a few draws at most"""
    from bootstrapper_amd.train import SyntheticSource
    src = SyntheticSource(CONFIGS["from_2d_mtlsd"], (40, 4, 4), 0, seed=42)
    for _ in range(3):
        lab, obf = src.labels()
        assert lab.dtype == obf.dtype == torch.int64 and tuple(lab.shape) == tuple(obf.shape) == (21, 100, 100)
        assert int(lab.min()) >= 0 and int(lab.max()) > 0


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_run_training_on_synthetic_labels(tmp_path, name):
    from bootstrapper_amd.train import latest_checkpoint, run_training
    setup = tmp_path / "setup_01"
    setup.mkdir()
    (setup / "net_config.json").write_text(json.dumps(CONFIGS[name]))
    cfg = tmp_path / "train.toml"
    cfg.write_text(f'setup_dir = "{setup}"\nvoxel_size = [40, 4, 4]\nmax_iterations = 3\nsave_checkpoints_every = 3\nsave_snapshots_every = 1000\n'
                   'synthetic_labels = true\n')
    logs = []
    assert run_training(str(cfg), log=logs.append) == 3
    ckpt, step = latest_checkpoint(str(setup))
    assert step == 3 and os.path.basename(ckpt) == "model_checkpoint_3.ckpt"
    losses = [float(l.split("train_loss")[1].split()[0].strip("=:, ")) for l in logs if "train_loss" in l]
    assert losses and all(math.isfinite(v) for v in losses)
    assert any("not built" in l and "DeformAugment" in l for l in logs)
