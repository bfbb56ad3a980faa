"""`bs train` with the train config key `augment`: SampleSource through the geometric chain on a small Zarr store written
here -- labels are boxes, raw is constant per label ((id * 37) % 256), so that any offset between the raw and the label
frame shows -- and five Trainer steps on 3d_affs at its smallest golden shape."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_ref as R  # noqa: E402

VOLUME, BOX = (36, 192, 192), (12, 32, 32)   # boxes of side >= 8; tests/test_aug_cpu.py checks the 20 % condition on this store
INPUT, OUTPUT = (14, 48, 48), (10, 32, 32)
VOXEL_SIZE = (40, 4, 4)
BATCHES = 6
# The alignment check concludes from "the 27 label samples around p fall into one box" that the 8 raw voxels around s(p) do.
# That holds where, on every axis, some neighbour's coordinate lies at least half a voxel below s(p) and another's above:
# in y and x the in-plane neighbours differ by u (|cos| + |sin|) >= 0.9 less the elastic slope (sigma 2 voxels over a spacing
# of 40: 0.07 per voxel); in z only if E_z is flat -- with the reference's z spacing of 4 voxels at sigma 2 the map folds
# along z as often as not, and a slip moves r across the in-plane gradient of E_z.  So this one test draws no z jitter; every
# other argument is the reference's, with deform and shift applied to every batch.
ALIGN = {"deform_p": 1.0, "shift_p": 1.0, "jitter_sigma": [0, 8, 8]}
NHOOD = [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]


def write_store(tmp_path, with_mask=False):
    from bootstrapper_amd.zarr_io import prepare_ds
    raw, labels = R.boxes_volume(VOLUME, BOX)
    store = str(tmp_path / "vol.zarr")
    arrays = [("raw", raw), ("labels", labels)] + ([("mask", (labels > 0).astype(np.uint8))] if with_mask else [])
    for name, arr in arrays:
        ds = prepare_ds(f"{store}/{name}", arr.shape, offset=(0, 0, 0), voxel_size=VOXEL_SIZE, chunk_shape=(12, 48, 48), dtype=arr.dtype)
        ds[:] = arr
    sample = {"raw": f"{store}/raw", "labels": f"{store}/labels"}
    if with_mask:
        sample["mask"] = f"{store}/mask"
    return [sample]


def source(samples, head="affs", augment=True, **kw):
    from bootstrapper_amd.train import SampleSource
    return SampleSource(samples, INPUT, OUTPUT, NHOOD, device=0, seed=42, head=head, voxel_size=VOXEL_SIZE, augment=augment, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("head,with_mask", [("affs", False), ("mtlsd", True)])
def test_augmented_source_keeps_keys_shapes_and_dtypes(tmp_path, head, with_mask):
    samples = write_store(tmp_path, with_mask)
    kw = {"lsd_sigma": 8.0, "lsd_downsample": 2} if head == "mtlsd" else {}
    plain, aug, aug2 = next(source(samples, head, None, **kw)), source(samples, head, True, **kw), source(samples, head, True, **kw)
    a = next(aug)
    assert set(a) == set(plain)
    for k in plain:
        assert a[k].shape == plain[k].shape and a[k].dtype == plain[k].dtype and a[k].device == plain[k].device, k
        assert bool(torch.isfinite(a[k]).all()), k
    assert not torch.equal(a["raw"], plain["raw"])                      # augmented differs from un-augmented
    b = next(aug2)
    assert all(torch.equal(a[k], b[k]) for k in a)                      # one seed, one sequence, bit for bit
    a, b = next(aug), next(aug2)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
def test_without_the_key_the_batches_are_those_of_the_plain_source(tmp_path):
    """augment=None takes no draw from the source's stream: same batches as a source built without the argument"""
    from bootstrapper_amd.train import SampleSource
    samples = write_store(tmp_path)
    old = SampleSource(samples, INPUT, OUTPUT, NHOOD, device=0, seed=42, voxel_size=VOXEL_SIZE)
    new = source(samples, augment=None)
    for _ in range(3):
        a, b = next(old), next(new)
        assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert old.rng.bit_generator.state == new.rng.bit_generator.state


@pytest.mark.gpu
def test_raw_and_labels_stay_aligned(tmp_path, monkeypatch):
    """At every output voxel whose 3 x 3 x 3 neighbourhood in the augmented labels is uniform and non-zero, raw is that
    label's value within the raw gate; such voxels are at least 20 % of the block."""
    from bootstrapper_amd import train as T
    samples = write_store(tmp_path)
    seen = []
    real = T.affinity_targets
    monkeypatch.setattr(T, "affinity_targets", lambda labels, *a, **k: (seen.append(labels.clone()), real(labels, *a, **k))[1])
    from bootstrapper_amd.augment import AugParams
    src = source(samples, augment=AugParams.from_config(ALIGN))   # grow_boundary = 0: the targets are made from the augmented labels
    ctx = [(i - o) // 2 for i, o in zip(INPUT, OUTPUT)]
    inner = tuple(slice(c, c + o) for c, o in zip(ctx, OUTPUT))
    for _ in range(BATCHES):
        batch = next(src)
        share, err = R.alignment(batch["raw"][inner].cpu().numpy(), seen[-1].cpu().numpy())
        print(f"alignment: {share:.3f} of the block checked, largest |raw - label value| {err:.3e}")
        assert share >= 0.2
        assert err <= R.RAW_GATE


def test_refusals_come_before_any_read():
    from bootstrapper_amd.train import SampleSource
    from bootstrapper_amd.augment import AugParams
    with pytest.raises(ValueError, match="square"):
        SampleSource([], (14, 48, 40), (10, 32, 24), NHOOD, augment=True)
    SampleSource([], (14, 48, 40), (10, 32, 24), NHOOD, augment=AugParams(simple=False))
    with pytest.raises(NotImplementedError, match="voxel_size"):
        SampleSource([], INPUT, OUTPUT, NHOOD, voxel_size=(40, 4, 8), augment=True)
    with pytest.raises(ValueError, match="LSD context"):
        SampleSource([], INPUT, OUTPUT, NHOOD, head="lsds", lsd_sigma=80.0, voxel_size=VOXEL_SIZE, augment=True)


@pytest.mark.gpu
def test_five_trainer_steps_with_augment(tmp_path):
    """`bs train` on 3d_affs at its smallest golden shape ((30, 108, 108) -> (2, 16, 16)) with `augment = true`"""
    from bootstrapper_amd.train import run_training
    from bootstrapper_amd.zarr_io import prepare_ds
    rng = np.random.default_rng(4)
    store = str(tmp_path / "vol.zarr")
    raw = rng.integers(0, 256, size=(40, 130, 130), dtype=np.uint8)
    labels = np.zeros((40, 130, 130), dtype=np.uint64)
    for i, (z, y, x) in enumerate(rng.integers(0, 100, size=(40, 3))):
        labels[z % 30:z % 30 + 10, y:y + 30, x:x + 30] = i + 1
    for name, arr in (("raw", raw), ("labels", labels)):
        ds = prepare_ds(f"{store}/{name}", arr.shape, offset=(0, 0, 0), voxel_size=(40, 4, 4), chunk_shape=(20, 64, 64), dtype=arr.dtype)
        ds[:] = arr
    setup = tmp_path / "setup_01"
    setup.mkdir()
    nc = {"in_channels": 1, "num_fmaps": 4, "fmap_inc_factor": 2, "downsample_factors": [[1, 2, 2]] * 3,
          "kernel_size_down": [[[3, 3, 3], [3, 3, 3]]] * 4, "kernel_size_up": [[[3, 3, 3], [3, 3, 3]]] * 3,
          "input_shape": [30, 108, 108], "output_shape": [2, 16, 16],
          "outputs": {"3d_affs": {"dims": 3, "neighborhood": NHOOD, "grow_boundary": 1}}}
    (setup / "net_config.json").write_text(json.dumps(nc))
    cfg = tmp_path / "train.toml"
    cfg.write_text(f'setup_dir = "{setup}"\nvoxel_size = [40, 4, 4]\nmax_iterations = 5\naugment = true\n'
                   f'[[samples]]\nraw = "{store}/raw"\nlabels = "{store}/labels"\n')
    logs = []
    assert run_training(str(cfg), log=logs.append) == 5
    losses = [float(l.split("train_loss")[1]) for l in logs if "train_loss" in l]    # "step N: train_loss X"
    assert len(losses) >= 1 and all(np.isfinite(losses)), logs
    assert any("geometric augmentation" in l and "NoiseAugment" in l for l in logs)
