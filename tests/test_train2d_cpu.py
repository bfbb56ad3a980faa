"""`bs train` on the 2-D setups, the host side: which sample source a setup gets and what its training step is."""
import json
import os

import numpy as np
import pytest

REF_2D = {"in_channels": 1, "adj_slices": 3, "num_fmaps": 12, "fmap_inc_factor": 5, "downsample_factors": [[2, 2], [2, 2], [2, 2]],
          "input_shape": [196, 196], "output_shape": [104, 104], "inputs": {"raw": {"dims": 1}}}
LSDS = {"dims": 6, "sigma": 80, "downsample": 2}
AFFS = {"dims": 6, "neighborhood": [[-1, 0], [0, -1], [-9, 0], [0, -9], [-27, 0], [0, -27]], "grow_boundary": 1}


def _config(tmp_path):
    from bootstrapper_amd.zarr_io import prepare_ds
    store = str(tmp_path / "s.zarr")
    for name, dtype in (("raw", np.uint8), ("labels", np.uint64)):
        prepare_ds(f"{store}/{name}", (4, 256, 256), offset=(0, 0, 0), voxel_size=(40, 4, 4), chunk_shape=(4, 128, 128), dtype=dtype)
    return {"samples": [{"raw": f"{store}/raw", "labels": f"{store}/labels"}], "voxel_size": [40, 4, 4]}


@pytest.mark.parametrize("outputs", [{"2d_lsds": LSDS, "2d_affs": AFFS}, {"2d_lsds": LSDS}, {"2d_affs": AFFS}])
def test_make_sample_source_builds_the_section_source(tmp_path, outputs):
    from bootstrapper_amd.train import SectionSource, make_sample_source
    nc = dict(REF_2D, outputs=outputs)
    src = make_sample_source(_config(tmp_path), nc, 0, 0)
    assert isinstance(src, SectionSource)
    assert src.batch_size == 10 and src.adj == 3 and src.out == (104, 104) and src.inp == (196, 196)
    if "2d_lsds" in outputs:
        assert src.lsd_ctx == [60, 60] and src.df == 2 and src.sigma == [80.0, 80.0]    # 3 sigma = 240 nm = 60 voxels of 4 nm
    if "2d_affs" in outputs:
        assert src.nhood[4] == [0, -27, 0] and src.aff_lo == [27, 27] and src.aff_hi == [0, 0] and src.grow == 1


def test_second_stage_setups_are_refused_by_name(tmp_path):
    from bootstrapper_amd.train import make_sample_source
    nc = {"num_fmaps": 12, "fmap_inc_factor": 5, "downsample_factors": [[1, 2, 2]] * 3, "input_shape": [24, 148, 148],
          "output_shape": [4, 56, 56], "inputs": {"2d_lsds": {"dims": 6}, "2d_affs": {"dims": 6}},
          "outputs": {"3d_affs": {"dims": 3, "neighborhood": [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]}}}
    with pytest.raises(NotImplementedError, match="3d_affs_from_2d_mtlsd"):
        make_sample_source(_config(tmp_path), nc, 0, 0)


def test_training_settings_follow_the_net_config():
    from bootstrapper_amd.train import training_settings
    s = training_settings(dict(REF_2D, outputs={"2d_lsds": LSDS}))
    assert s == {"two_d": True, "batch_size": 10, "in_shape": (10, 196, 196), "lr": 1.0e-4}
    s = training_settings({"downsample_factors": [[1, 2, 2]] * 3, "input_shape": [32, 196, 196], "outputs": {"3d_affs": {"dims": 3}}})
    assert s == {"two_d": False, "batch_size": 1, "in_shape": (32, 196, 196), "lr": 0.5e-4}


def test_stacked_sections_put_the_batch_axis_first():
    import torch
    from bootstrapper_amd.training import stacked_sections
    data = {"raw": torch.zeros(3, 10, 196, 196), "gt_lsds": torch.zeros(6, 10, 104, 104), "pred_affs": torch.zeros(6, 10, 104, 104)}
    out = stacked_sections(data)
    assert tuple(out["raw"].shape) == (10, 3, 196, 196)
    assert tuple(out["gt_lsds"].shape) == (10, 6, 1, 104, 104) and tuple(out["pred_affs"].shape) == (10, 6, 1, 104, 104)


def test_lsd2d_restatement_basics():
    """tests/lsd2d_ref.py on a disc: background is 0, the disc's centre has offset 0.5 and equal variances"""
    from lsd2d_ref import lsd2d_targets
    yy, xx = np.mgrid[:64, :64]
    lab = ((yy - 32) ** 2 + (xx - 32) ** 2 < 15 ** 2).astype(np.int64)[None]
    d, w = lsd2d_targets(lab, (16, 16), (32, 32), (20.0, 20.0), (2.0, 2.0), 1)
    assert d.shape == (6, 1, 32, 32) and (d[:, lab[:, 16:48, 16:48] == 0] == 0).all()
    c = d[:, 0, 16, 16]
    assert abs(c[0] - 0.5) < 1e-6 and abs(c[1] - 0.5) < 1e-6 and abs(c[2] - c[3]) < 1e-6 and abs(c[4] - 0.5) < 1e-6
    assert w.shape == (6, 1, 32, 32)


def test_stacked_snapshot_is_written(tmp_path):
    """the snapshot of a 2-D batch holds five-axis arrays (batch, C, 1, h, w), which the Zarr writer takes"""
    import torch
    from bootstrapper_amd.training import save_snapshot, stacked_sections
    from bootstrapper_amd.zarr_io import open_ds
    g = torch.Generator().manual_seed(0)
    data = {"raw": torch.rand(3, 10, 36, 36, generator=g) * 2 - 1, "gt_lsds": torch.rand(6, 10, 16, 16, generator=g),
            "pred_lsds": torch.rand(6, 10, 16, 16, generator=g)}
    path = save_snapshot(str(tmp_path), (40, 4, 4), 1, 0, stacked_sections(data))
    pred = open_ds(path + "/pred_lsds")
    assert pred.shape == (10, 6, 1, 16, 16) and open_ds(path + "/raw").shape == (10, 3, 36, 36)
    assert np.array_equal(pred[:], data["pred_lsds"].transpose(0, 1)[:, :, None].numpy())
