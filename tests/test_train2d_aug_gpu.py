"""`bs train` on the 2-D setups with the train config key `augment2d`: SectionSource through the batched geometric chain on
a small Zarr store written here -- labels are boxes, raw is constant per label ((id * 37) % 256), so that any offset between
the raw and the label frame shows; the LSD context (30 pixels) exceeds the network's (8), so the labels are sampled beyond
the input section -- and five Trainer steps of a small 2d_mtlsd net."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug2d_ref as R  # noqa: E402
import aug_ref  # noqa: E402

VOLUME, BOX = (36, 192, 192), (12, 32, 32)   # tests/test_aug2d_cpu.py checks the 20 % condition on this store
INPUT, OUTPUT, ADJ = (48, 48), (32, 32), 3
VOXEL_SIZE = (40, 4, 4)
LSDS = {"dims": 6, "sigma": 40, "downsample": 1}   # 3 sigma / 4 nm: a context of 30 pixels
AFFS = {"dims": 2, "neighborhood": [[-1, 0], [0, -1]], "grow_boundary": 0}   # 0: the targets are made from the augmented labels as they are
BATCHES = 6
# The alignment check concludes from "the 9 label samples around p fall into one box" that the 4 raw pixels around s(p) do.
# That holds where, on both axes, some neighbour's coordinate lies at least half a pixel below s(p) and another's above: the
# in-plane neighbours differ by u (|cos| + |sin|) >= 0.9 less the elastic slope (sigma 2 pixels over a spacing of 40: 0.07
# per pixel).  z is never interpolated, and raw's centre section takes the shift the labels take, so every argument is the
# reference's, with the deformation applied to every draw.
ALIGN = {"deform_p": 1.0}


def label_margins():
    """SectionSource's lo = hi for LSDS and AFFS at VOXEL_SIZE: the larger of the LSD context and the neighbourhood's"""
    return (30, 30)


def write_store(tmp_path, with_mask=False):
    from bootstrapper_amd.zarr_io import prepare_ds
    raw, labels = aug_ref.boxes_volume(VOLUME, BOX)
    store = str(tmp_path / "vol.zarr")
    arrays = [("raw", raw), ("labels", labels)] + ([("mask", (labels > 0).astype(np.uint8))] if with_mask else [])
    for name, arr in arrays:
        ds = prepare_ds(f"{store}/{name}", arr.shape, offset=(0, 0, 0), voxel_size=VOXEL_SIZE, chunk_shape=(12, 48, 48), dtype=arr.dtype)
        ds[:] = arr
    sample = {"raw": f"{store}/raw", "labels": f"{store}/labels"}
    if with_mask:
        sample["mask"] = f"{store}/mask"
    return [sample]


def source(samples, **kw):
    from bootstrapper_amd.train import SectionSource
    return SectionSource(samples, INPUT, OUTPUT, ADJ, device=0, seed=42, batch_size=10, lsds=LSDS, affs=AFFS, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("with_mask", [False, True])
def test_augmented_source_keeps_keys_shapes_and_dtypes(tmp_path, with_mask):
    samples = write_store(tmp_path, with_mask)
    plain, aug, aug2 = next(source(samples)), source(samples, augment=True), source(samples, augment=True)
    assert (aug.lo, aug.hi) == (list(label_margins()),) * 2 and aug.frame == ((-22, -22), (70, 70))   # the labels reach beyond the input section
    a = next(aug)
    assert list(a) == list(plain)
    for k in plain:
        assert a[k].shape == plain[k].shape and a[k].dtype == plain[k].dtype and a[k].device == plain[k].device, k
        assert a[k].is_contiguous() == plain[k].is_contiguous() and bool(torch.isfinite(a[k]).all()), k
    assert not torch.equal(a["raw"], plain["raw"])                      # augmented differs from un-augmented
    b = next(aug2)
    assert all(torch.equal(a[k], b[k]) for k in a)                      # one seed, one sequence, bit for bit
    a, b = next(aug), next(aug2)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert aug.rng.bit_generator.state == aug2.rng.bit_generator.state


@pytest.mark.gpu
def test_without_the_key_the_batches_are_those_of_the_plain_source(tmp_path):
    """augment=None takes no draw from the source's stream: same batches as a source built without the argument"""
    samples = write_store(tmp_path)
    old, new = source(samples), source(samples, augment=None)
    for _ in range(3):
        a, b = next(old), next(new)
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert old.rng.bit_generator.state == new.rng.bit_generator.state


@pytest.mark.gpu
def test_raw_and_labels_stay_aligned(tmp_path, monkeypatch):
    """At every output pixel whose 3 x 3 neighbourhood in the augmented labels is uniform and non-zero, raw's centre channel
    is that label's value within the raw gate; such pixels are at least 20 % of every batch."""
    from bootstrapper_amd import train as T
    from bootstrapper_amd.augment2d import Aug2DParams
    samples = write_store(tmp_path)
    seen = []
    real = T.lsd2d_targets
    monkeypatch.setattr(T, "lsd2d_targets", lambda labels, *a, **k: (seen.append(labels.clone()), real(labels, *a, **k))[1])
    src = source(samples, augment=Aug2DParams.from_config(ALIGN))
    m, c = label_margins(), [(i - o) // 2 for i, o in zip(INPUT, OUTPUT)]
    for _ in range(BATCHES):
        batch = next(src)
        labels = seen[-1][:, m[0]:m[0] + OUTPUT[0], m[1]:m[1] + OUTPUT[1]].cpu().numpy()     # the LSD call takes the whole labels window
        raw = batch["raw"][ADJ // 2, :, c[0]:c[0] + OUTPUT[0], c[1]:c[1] + OUTPUT[1]].cpu().numpy()
        share, err = R.alignment(raw, labels)
        print(f"alignment: {share:.3f} of the batch checked, largest |raw - label value| {err:.3e} (gate {R.RAW_GATE:.3e})")
        assert share >= 0.2
        assert err <= R.RAW_GATE


def test_refusals_come_before_any_read():
    from bootstrapper_amd.augment2d import Aug2DParams
    from bootstrapper_amd.train import SectionSource
    with pytest.raises(ValueError, match="square"):
        SectionSource([], (48, 40), (32, 24), ADJ, lsds=LSDS, augment=True)
    with pytest.raises(ValueError, match="square"):
        SectionSource([], (48, 48), (32, 24), ADJ, lsds=LSDS, augment=Aug2DParams(deform_p=0.0))


def test_rotation_on_an_anisotropic_section_grid_is_refused(tmp_path):
    """the voxel size is the store's metadata: the source refuses after opening the datasets and before reading from them"""
    from bootstrapper_amd.augment2d import Aug2DParams
    from bootstrapper_amd.train import SectionSource
    from bootstrapper_amd.zarr_io import prepare_ds
    store = str(tmp_path / "vol.zarr")
    for name, dtype in (("raw", np.uint8), ("labels", np.uint64)):
        prepare_ds(f"{store}/{name}", (4, 80, 80), offset=(0, 0, 0), voxel_size=(40, 4, 8), chunk_shape=(4, 80, 80), dtype=dtype)
    samples = [{"raw": f"{store}/raw", "labels": f"{store}/labels"}]
    with pytest.raises(NotImplementedError, match="voxel_size"):
        SectionSource(samples, INPUT, OUTPUT, ADJ, lsds=LSDS, augment=True)
    assert SectionSource(samples, INPUT, OUTPUT, ADJ, lsds=LSDS, augment=Aug2DParams(rotate=False)).augment.rotate is False


@pytest.mark.gpu
def test_five_trainer_steps_with_augment2d(tmp_path):
    """`bs train` on a small 2d_mtlsd net ((108, 108) -> (16, 16), adj_slices 3, the shipped sigma of 80: a context of 60 pixels
    against the network's 46) with `augment2d = true`"""
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
    cfg.write_text(f'setup_dir = "{setup}"\nvoxel_size = [40, 4, 4]\nmax_iterations = 5\naugment2d = true\n'
                   f'[[samples]]\nraw = "{samples[0]["raw"]}"\nlabels = "{samples[0]["labels"]}"\n')
    logs = []
    assert run_training(str(cfg), log=logs.append) == 5
    losses = [float(l.split("train_loss")[1]) for l in logs if "train_loss" in l]    # "step N: train_loss X"
    assert len(losses) >= 1 and all(np.isfinite(losses)), logs
    assert any("geometric augmentation of the 2-D setups" in l and "augment2d" in l and "NoiseAugment" in l for l in logs)
