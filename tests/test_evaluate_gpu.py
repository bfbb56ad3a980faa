"""`bs evaluate` on the MI355X: the error kernels bit-equal to the restatement (tests/eval_ref.py), the contingency table equal
to np.unique, Rand / VOI, and both modes end to end through the command line on a small store."""
import json
import os

import numpy as np
import pytest

import eval_ref as R

pytestmark = pytest.mark.gpu

NEG = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -8, 0], [0, 0, -8]]


def _ds(path, a, offset=(0, 0, 0), voxel_size=(1, 1, 1), chunk=None):
    from bootstrapper_amd.zarr_io import prepare_ds
    d = prepare_ds(path, a.shape, offset=offset, voxel_size=voxel_size, chunk_shape=chunk or a.shape, dtype=a.dtype,
                   axis_names=(["c^"] if a.ndim == 4 else []) + ["z", "y", "x"], units=["nm"] * 3)
    d[:] = a
    return d


def _blobs(rng, shape, n, lo=1):
    """Voronoi-like ids: every voxel takes the id of its nearest of n random seeds"""
    pts = np.stack([rng.integers(0, s, n) for s in shape], 1)
    ids = rng.integers(lo, lo + 10 * n, n).astype(np.uint64)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3)
    d = ((grid[:, None, :] - pts[None, :, :]) ** 2 * np.array([16, 1, 1])).sum(-1)
    return ids[np.argmin(d, 1)].reshape(shape)


@pytest.fixture(scope="module")
def engine():
    from bootstrapper_amd.evaluate import EvalDevice
    e = EvalDevice(0)
    yield e
    e.close()


def _case(tmp_path, name, seg, seg_offset, pred, pred_offset, mask=None, chunk=(10, 32, 32)):
    store = str(tmp_path / f"{name}.zarr")
    vs = (4, 2, 2)
    s = _ds(store + "/seg", seg, offset=[o * v for o, v in zip(seg_offset, vs)], voxel_size=vs, chunk=(8, 16, 16))
    p = _ds(store + "/pred/3d_affs", pred, offset=[o * v for o, v in zip(pred_offset, vs)], voxel_size=vs, chunk=(pred.shape[0],) + chunk)
    m = None if mask is None else _ds(store + "/mask", mask, offset=[o * v for o, v in zip(pred_offset, vs)], voxel_size=vs).path
    return store, s.path, p.path, m


def _run(engine, store, seg, pred, mask, nhood, whole_roi=False, thresholds=(0.1, 1.0)):
    from bootstrapper_amd.evaluate import compute_errors
    from bootstrapper_amd.zarr_io import open_ds
    outs = [(store + "/out/error_map", store + "/out/error_mask")]
    stats = compute_errors([seg], pred, mask, outs, thresholds=thresholds, aff_neighborhood=nhood, engine=engine, whole_roi=whole_roi)
    return open_ds(outs[0][0]), open_ds(outs[0][1]), stats[0]


@pytest.mark.parametrize("nhood", [R.DEFAULT_NEIGHBORHOOD, NEG], ids=["positive", "negative"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_errors_bit_equal_to_restatement(tmp_path, engine, nhood, masked):
    """ROI (23, 50, 61) inside a larger seg dataset (the halo reads real ids), chunks (10, 32, 32) overlapping on every axis"""
    rng = np.random.default_rng(11)
    seg = _blobs(rng, (29, 64, 80), 40)
    seg[rng.random(seg.shape) < 0.02] = 0
    pred = rng.integers(0, 256, (6, 23, 50, 61), dtype=np.uint8)
    pred[:, 3:6] = np.where(rng.random((6, 3, 50, 61)) < 0.5, 255, 0).astype(np.uint8)
    mask = rng.integers(0, 3, (23, 50, 61)).astype(np.uint8) if masked else None
    store, s, p, m = _case(tmp_path, "c", seg, (0, 0, 0), pred, (3, 7, 9), mask)
    emap, emask, stats = _run(engine, store, s, p, m, nhood)
    ref_map, ref_mask = R.aff_errors(seg, (3, 7, 9), pred, nhood, (10, 32, 32), mask=mask)
    assert emap.shape == (23, 50, 61) and emap.dtype == np.uint8 and emap.offset == (12, 14, 18) and emap.voxel_size == (4, 2, 2)
    got_map, got_mask = emap[:], emask[:]
    assert np.array_equal(got_map, ref_map), int((got_map != ref_map).sum())
    assert np.array_equal(got_mask, ref_mask), int((got_mask != ref_mask).sum())
    for got, ref in zip(stats, (R.compute_stats(ref_map), R.compute_stats(ref_mask))):
        assert got["mean"] == ref["mean"] and got["num_nonzero_voxels"] == ref["num_nonzero_voxels"]
        assert got["total_voxels"] == ref["total_voxels"] and abs(got["std"] - ref["std"]) <= 1e-12 * max(1.0, ref["std"])
    # the whole ROI as one tile gives the same outputs
    emap2, emask2, stats2 = _run(engine, store, s, p, m, nhood, whole_roi=True)
    assert np.array_equal(emap2[:], ref_map) and np.array_equal(emask2[:], ref_mask) and stats2 == stats


def test_errors_at_the_dataset_edge_and_an_all_zero_chunk(tmp_path, engine):
    """ROI = the whole seg dataset: neighbours beyond it read 0; one chunk holds no error at all (max 0 -> 0)"""
    rng = np.random.default_rng(12)
    seg = _blobs(rng, (23, 50, 61), 30)
    pred = rng.integers(0, 256, (6, 23, 50, 61), dtype=np.uint8)
    seg[:10, :32, :32] = 0          # the first chunk: no ids, no affinity, so diff = 0 everywhere in it
    pred[:, :10, :32, :32] = 0
    store, s, p, m = _case(tmp_path, "e", seg, (0, 0, 0), pred, (0, 0, 0))
    emap, emask, _ = _run(engine, store, s, p, m, NEG, thresholds=(0.05, 0.9))
    ref_map, ref_mask = R.aff_errors(seg, (0, 0, 0), pred, NEG, (10, 32, 32), thresholds=(0.05, 0.9))
    assert not ref_map[:10, :18, :29].any()
    assert np.array_equal(emap[:], ref_map) and np.array_equal(emask[:], ref_mask)
    emap, emask, _ = _run(engine, store, s, p, m, R.DEFAULT_NEIGHBORHOOD)
    ref_map, ref_mask = R.aff_errors(seg, (0, 0, 0), pred, R.DEFAULT_NEIGHBORHOOD, (10, 32, 32))
    assert np.array_equal(emap[:], ref_map) and np.array_equal(emask[:], ref_mask)


@pytest.mark.parametrize("channels", [3, 4])
def test_errors_other_channel_counts(tmp_path, engine, channels):
    """pred datasets with fewer channels than the neighbourhood: the neighbourhood is truncated (3 and 6 channels take
    kernels specialised on the count, any other count the generic one)"""
    rng = np.random.default_rng(16 + channels)
    seg = _blobs(rng, (20, 40, 45), 25)
    pred = rng.integers(0, 256, (channels, 17, 33, 37), dtype=np.uint8)
    mask = rng.integers(0, 2, (17, 33, 37)).astype(np.uint8)
    store, s, p, m = _case(tmp_path, "k", seg, (0, 0, 0), pred, (2, 3, 4), mask, chunk=(7, 16, 16))
    emap, emask, _ = _run(engine, store, s, p, m, NEG)
    ref_map, ref_mask = R.aff_errors(seg, (2, 3, 4), pred, NEG, (7, 16, 16), mask=mask)
    assert np.array_equal(emap[:], ref_map) and np.array_equal(emask[:], ref_mask)


def _pairs(engine, gt, seg, mask=None):
    from bootstrapper_amd.evaluate import merge_pairs
    return merge_pairs([engine.pairs(engine.to_dev(gt), engine.to_dev(seg), None if mask is None else engine.to_dev(mask))])


def test_contingency_counts_equal_unique(engine):
    rng = np.random.default_rng(13)
    shape = (9, 70, 130)
    gt = _blobs(rng, shape, 25)
    seg = _blobs(rng, shape, 60)
    gt[rng.random(shape) < 0.05] = 0
    big = np.array([2**32, 2**32 + 1, 2**63 + 5, 2**64 - 2, 2**64 - 1], np.uint64)
    seg[rng.random(shape) < 0.05] = 0
    sel = rng.random(shape) < 0.1
    seg[sel] = big[rng.integers(0, 5, int(sel.sum()))]
    sel = rng.random(shape) < 0.1
    gt[sel] = big[rng.integers(0, 5, int(sel.sum()))]
    for mask in (None, rng.integers(0, 3, shape).astype(np.uint8)):
        g, s, n = _pairs(engine, gt, seg, mask)
        rg, rs, rn = R.contingency(gt, seg, mask)
        assert np.array_equal(g, rg) and np.array_equal(s, rs) and np.array_equal(n, rn)
    assert (g >= 2**64 - 2).any() and (s == 2**64 - 1).any()


def test_undersized_table_reports_overflow():
    from bootstrapper_amd import _lib
    from bootstrapper_amd.evaluate import EvalDevice
    small = EvalDevice(0, pair_capacity=16)
    try:
        gt = np.arange(1, 201, dtype=np.uint64).reshape(2, 10, 10)
        with pytest.raises(_lib.BsmiError) as e:
            small.pairs(small.to_dev(gt), small.to_dev(gt), None)
        assert e.value.code == _lib.ERR_OVERFLOW and "overflow" in e.value.msg
        ok = np.ones((2, 10, 10), np.uint64)     # the flag was cleared by the status read: a small tile passes again
        g, s, n = small.pairs(small.to_dev(ok), small.to_dev(ok), None)
        assert g.tolist() == [1] and n.tolist() == [200]
    finally:
        small.close()


def test_metrics_match_restatement(tmp_path, engine):
    from bootstrapper_amd.evaluate import compute_metrics
    rng = np.random.default_rng(14)
    gt = _blobs(rng, (12, 40, 50), 20)
    gt[:, :5] = 0
    seg = _blobs(rng, (12, 40, 50), 35)
    mask = (rng.random((12, 40, 50)) < 0.9).astype(np.uint8)
    store = str(tmp_path / "m.zarr")
    _ds(store + "/gt", gt)
    _ds(store + "/seg", seg)
    _ds(store + "/mask", mask)
    for m in (None, mask):
        got = compute_metrics(store + "/seg", store + "/gt", None if m is None else store + "/mask", engine=engine, tile_voxels=5000)
        ref = R.rand_voi(gt, seg, m)
        assert list(got["voi"]) == list(ref)
        for k, v in ref.items():
            assert abs(got["voi"][k] - v) <= 1e-12 * max(1.0, abs(v)), (k, got["voi"][k], v)


def test_evaluate_end_to_end(tmp_path):
    """`eval` through the command line in both modes over two segmentations written by `run_segmentation`"""
    from click.testing import CliRunner
    from scipy.ndimage import gaussian_filter
    from bootstrapper_amd.cli import cli
    from bootstrapper_amd.segment import run_segmentation
    from bootstrapper_amd.zarr_io import open_ds
    rng = np.random.default_rng(15)
    shape = (23, 50, 61)
    a = gaussian_filter(rng.random((6,) + shape), sigma=(0, 1, 2, 2))
    affs = ((a - a.min()) / (a.max() - a.min()) * 255).astype(np.uint8)
    store = str(tmp_path / "vol.zarr")
    vs = (40, 4, 4)
    _ds(store + "/predictions/3d_affs", affs, offset=(80, 8, 8), voxel_size=vs, chunk=(6, 10, 32, 32))
    gt = _blobs(rng, shape, 15)
    _ds(store + "/labels", gt, offset=(80, 8, 8), voxel_size=vs, chunk=(8, 32, 32))
    mask = np.ones(shape, np.uint8)
    mask[:, :, :6] = 0
    _ds(store + "/mask", mask, offset=(80, 8, 8), voxel_size=vs, chunk=(8, 32, 32))
    seg_cfg = tmp_path / "seg.toml"
    seg_cfg.write_text(f'''affs_dataset = "{store}/predictions/3d_affs"
fragments_dataset = "{store}/fragments"
seg_dataset_prefix = "{store}/segmentations"
blockwise = false
[ws_params]
thresholds = [0.3, 0.6]
min_seed_distance = 4
''')
    written = run_segmentation(str(seg_cfg), "ws")
    segs = written[1:]
    assert len(segs) == 2
    cfg = tmp_path / "04_eval_vol.toml"
    cfg.write_text(f'''seg_datasets_prefix = "{store}/segmentations"
mask_dataset = "{store}/mask"
[gt]
labels_dataset = "{store}/labels"
[pred]
pred_dataset = "{store}/predictions/3d_affs"
thresholds = [0.1, 0.9]
[pred.params]
aff_neighborhood = {NEG}
''')
    r = CliRunner().invoke(cli, ["eval", str(cfg)])
    assert r.exit_code == 0, (r.output, r.exception)
    res_pred = json.loads((tmp_path / "results_pred_vol.json").read_text())
    res_gt = json.loads((tmp_path / "results_gt_vol.json").read_text())
    assert list(res_pred) == segs and list(res_gt) == segs
    for sp in segs:
        seg = open_ds(sp)[:]
        e = res_pred[sp]
        assert list(e) == ["seg_ds", "pred_ds", "mask_ds", "map_ds", "thresholds", "error_map", "error_mask"]
        assert e["mask_ds"] == sp + "__vs__3d_affs/error_mask" and e["map_ds"] == sp + "__vs__3d_affs/error_map"
        assert e["pred_ds"] == store + "/predictions/3d_affs" and e["thresholds"] == [0.1, 0.9]
        ref_map, ref_mask = R.aff_errors(seg, (0, 0, 0), affs, NEG, (10, 32, 32), (0.1, 0.9), mask)
        for key, ref in (("error_map", ref_map), ("error_mask", ref_mask)):
            d = open_ds(e["map_ds" if key == "error_map" else "mask_ds"])
            assert d.dtype == np.uint8 and d.offset == (80, 8, 8) and d.voxel_size == vs and d.axis_names == ["z", "y", "x"]
            assert np.array_equal(d[:], ref), key
            st, rs = e[key], R.compute_stats(ref)
            assert st["mean"] == rs["mean"] and st["num_nonzero_voxels"] == rs["num_nonzero_voxels"]
            assert st["total_voxels"] == rs["total_voxels"] and st["nonzero_ratio"] == rs["nonzero_ratio"]
            assert abs(st["std"] - rs["std"]) <= 1e-12 * max(1.0, rs["std"])
        g = res_gt[sp]
        assert list(g) == ["seg_ds", "labels_ds", "skeletons_file", "mask_ds", "metrics"]
        assert g["mask_ds"] == store + "/mask" and g["skeletons_file"] is None and g["labels_ds"] == store + "/labels"
        ref = R.rand_voi(gt, seg, mask)
        for k, v in ref.items():
            assert abs(g["metrics"]["voi"][k] - v) <= 1e-12 * max(1.0, abs(v)), k
    # a second run skips the error datasets it wrote; -p alone writes only the pred results
    os.remove(tmp_path / "results_gt_vol.json")
    r = CliRunner().invoke(cli, ["evaluate", str(cfg), "-p", "-o", str(tmp_path / "again.json")])
    assert r.exit_code == 0, (r.output, r.exception)
    assert json.loads((tmp_path / "again.json").read_text()) == res_pred
    assert not (tmp_path / "results_gt_vol.json").exists()
