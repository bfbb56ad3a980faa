"""`bs train` with `intensity` inside the `[augment]` table: SampleSource through the geometric and the intensity chain on a
small Zarr store written here, and five Trainer steps on 3d_affs at its smallest golden shape."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_ref  # noqa: E402
from bootstrapper_amd import augment as A  # noqa: E402

pytestmark = pytest.mark.gpu

VOLUME, BOX = (36, 192, 192), (12, 32, 32)
INPUT, OUTPUT = (14, 48, 48), (10, 32, 32)
VOXEL_SIZE = (40, 4, 4)
NHOOD = [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]


@pytest.fixture(scope="module")
def samples(tmp_path_factory):
    from bootstrapper_amd.zarr_io import prepare_ds
    raw, labels = aug_ref.boxes_volume(VOLUME, BOX)
    store = str(tmp_path_factory.mktemp("store") / "vol.zarr")
    for name, arr in (("raw", raw), ("labels", labels), ("mask", (labels > 0).astype(np.uint8))):
        ds = prepare_ds(f"{store}/{name}", arr.shape, offset=(0, 0, 0), voxel_size=VOXEL_SIZE, chunk_shape=(12, 48, 48), dtype=arr.dtype)
        ds[:] = arr
    return [{"raw": f"{store}/raw", "labels": f"{store}/labels", "mask": f"{store}/mask"}]


def source(samples, augment, head="mtlsd"):
    from bootstrapper_amd.train import SampleSource
    kw = {"lsd_sigma": 8.0, "lsd_downsample": 2} if head == "mtlsd" else {}
    return SampleSource(samples, INPUT, OUTPUT, NHOOD, device=0, seed=42, head=head, voxel_size=VOXEL_SIZE, augment=augment, **kw)


def params(**intensity):
    return A.AugParams.from_config({"intensity": intensity or True})


def same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_keys_shapes_dtypes_and_one_seed_one_sequence(samples):
    plain, one, two = source(samples, True), source(samples, params()), source(samples, params())
    differs = False
    for _ in range(4):
        g, a, b = next(plain), next(one), next(two)
        assert set(a) == set(g)
        for k in g:
            assert a[k].shape == g[k].shape and a[k].dtype == g[k].dtype and a[k].device == g[k].device, k
            assert bool(torch.isfinite(a[k]).all()), k
        assert same(a, b)                                                  # bit for bit
        assert float(a["raw"].min()) >= -1.0 and float(a["raw"].max()) <= 1.0
        differs |= not torch.equal(a["raw"], g["raw"])
    assert differs                                                         # the chain did something (each batch: with probability 0.98)


def test_without_intensity_the_batches_are_the_geometric_ones(samples):
    old, new = source(samples, True), source(samples, A.AugParams.from_config({"intensity": False}))
    for _ in range(3):
        assert same(next(old), next(new))
    assert old.rng.bit_generator.state == new.rng.bit_generator.state


def test_a_plan_without_an_applied_node_is_sample_raw(samples):
    """every node off: the intensity plan takes no draw and applies nothing, so the batches are the geometric ones, bit for bit"""
    off = params(noise_p=0, intensity_p=0, gamma_p=0, impulse_p=0, smooth_p=0, prob_missing=0, prob_low_contrast=0)
    old, new = source(samples, True), source(samples, off)
    for _ in range(3):
        assert same(next(old), next(new))
    assert old.rng.bit_generator.state == new.rng.bit_generator.state


def test_missing_sections_touch_raw_alone(samples):
    """prob_missing = 1: every section of raw is constant -1 or +1; labels and targets are those of prob_missing = 0 (the draws
    of the defect node do not depend on their outcome, so the two streams stay together)"""
    gone, kept = source(samples, params(prob_missing=1.0, prob_low_contrast=0.0)), source(samples, params(prob_missing=0.0))
    values = set()
    for _ in range(3):
        a, b = next(gone), next(kept)
        raw = a["raw"]
        first = raw[:, :1, :1]
        assert bool((raw == first).all()) and bool(((first == 1) | (first == -1)).all())
        values |= set(first.flatten().tolist())
        assert all(torch.equal(a[k], b[k]) for k in a if k != "raw")
        assert not torch.equal(a["raw"], b["raw"])
    assert values == {-1.0, 1.0}                                           # 42 sections, each value with probability 1/2


def test_five_trainer_steps_with_intensity(tmp_path):
    """`bs train` on 3d_affs at its smallest golden shape ((30, 108, 108) -> (2, 16, 16)) with the intensity chain alone"""
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
    # the geometric nodes switched off in the table: the intensity chain without geometry
    cfg.write_text(f'setup_dir = "{setup}"\nvoxel_size = [40, 4, 4]\nmax_iterations = 5\n'
                   f'[[samples]]\nraw = "{store}/raw"\nlabels = "{store}/labels"\n'
                   '[augment]\nsimple = false\ndeform_p = 0\nshift_p = 0\n[augment.intensity]\nnoise_p = 1.0\nsmooth_p = 1.0\n')
    logs = []
    assert run_training(str(cfg), log=logs.append) == 5
    losses = [float(l.split("train_loss")[1]) for l in logs if "train_loss" in l]
    assert len(losses) >= 1 and all(np.isfinite(losses)), logs
    assert any("intensity chain" in l and "NoiseAugment" in l and "artifacts" in l for l in logs)
