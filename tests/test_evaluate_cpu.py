"""`bs evaluate` host logic: command line, modes, config defaults, dataset discovery, refusals, and the restatement's hand-computed
cases (tests/eval_ref.py).  No GPU."""
import json
import os

import numpy as np
import pytest
from click.testing import CliRunner

import eval_ref as R


def _ds(path, a, offset=(0, 0, 0), voxel_size=(1, 1, 1), chunk=None):
    from bootstrapper_amd.zarr_io import prepare_ds
    nd = 3
    d = prepare_ds(path, a.shape, offset=offset, voxel_size=voxel_size, chunk_shape=chunk or a.shape, dtype=a.dtype,
                   axis_names=(["c^"] if a.ndim == 4 else []) + ["z", "y", "x"][-nd:], units=["nm"] * nd)
    d[:] = a
    return d


def test_help_lists_evaluate_and_its_flags():
    from bootstrapper_amd.cli import cli
    r = CliRunner().invoke(cli, ["--help"])
    assert r.exit_code == 0 and "evaluate" in r.output and "eval " in r.output
    for name in ("evaluate", "eval"):
        r = CliRunner().invoke(cli, [name, "--help"])
        assert r.exit_code == 0, r.output
        for flag in ("--gt", "-gt", "--pred", "-p", "--out_result", "-o"):
            assert flag in r.output, (name, flag)


def test_mode_selection(tmp_path):
    from bootstrapper_amd.evaluate import eval_modes
    cfg = tmp_path / "04_eval_v.toml"
    cfg.write_text('seg_datasets_prefix = "x"\n')
    assert eval_modes(str(cfg)) == ["pred"]
    cfg.write_text('seg_datasets_prefix = "x"\n[pred]\npred_dataset = "p/3d_affs"\n[gt]\nlabels_dataset = "g"\n')
    assert eval_modes(str(cfg)) == ["gt", "pred"]
    assert eval_modes(str(cfg), gt=True) == ["gt"]
    assert eval_modes(str(cfg), pred=True) == ["pred"]
    assert eval_modes(str(cfg), gt=True, pred=True) == ["gt", "pred"]
    cfg.write_text('[gt]\nlabels_dataset = "g"\n')
    assert eval_modes(str(cfg)) == ["gt"]


def test_default_out_result_and_overrides(tmp_path):
    from bootstrapper_amd.evaluate import get_eval_config
    cfg = tmp_path / "04_eval_vol.toml"
    cfg.write_text('seg_datasets_prefix = "x"\n')
    assert get_eval_config(str(cfg), "pred")["out_result"] == str(tmp_path / "results_pred_vol.json")
    assert get_eval_config(str(cfg), "gt")["out_result"] == str(tmp_path / "results_gt_vol.json")
    c = get_eval_config(str(cfg), "gt", out_result="o.json", seg_datasets_prefix=None)
    assert c["out_result"] == "o.json" and c["seg_datasets_prefix"] == "x"


def test_refuses_to_overwrite_the_config(tmp_path):
    from bootstrapper_amd.evaluate import run_evaluation
    cfg = tmp_path / "evaluation.cfg"      # neither 04_eval_ nor .toml: the reference's default name is the config itself
    cfg.write_text('seg_datasets = []\n[pred]\npred_dataset = "a.zarr/3d_affs"\n')
    before = cfg.read_text()
    with pytest.raises(ValueError, match="would overwrite the config file"):
        run_evaluation(str(cfg), "pred")
    assert cfg.read_text() == before


def test_seg_dataset_discovery_skips_error_datasets(tmp_path):
    from bootstrapper_amd.evaluate import get_seg_datasets
    root = tmp_path / "v.zarr"
    for p in ("segs/ws--t0.5", "segs/ws--t0.3", "segs_b/cc", "segs__vs__3d_affs/error_map", "segs/ws--t0.3__vs__3d_affs",
              "segs/ws--t0.3__vs__3d_affs/error_map", "other/x"):
        (root / p).mkdir(parents=True, exist_ok=True)
        (root / p / ".zarray").write_text("{}")
    got = get_seg_datasets(str(root / "segs"))
    assert got == [str(root / "segs/ws--t0.3"), str(root / "segs/ws--t0.5"), str(root / "segs_b/cc")]


def test_lsd_datasets_and_skeletons_are_refused(tmp_path):
    from bootstrapper_amd.evaluate import run_evaluation
    cfg = tmp_path / "04_eval_v.toml"
    cfg.write_text(f'seg_datasets = ["{tmp_path}/v.zarr/seg"]\n[pred]\npred_dataset = "{tmp_path}/v.zarr/pred/3d_lsds"\n')
    with pytest.raises(NotImplementedError, match="3d_lsds"):
        run_evaluation(str(cfg), "pred")
    cfg.write_text(f'seg_datasets = ["{tmp_path}/v.zarr/seg"]\n[gt]\nskeletons_file = "{tmp_path}/skel.graphml"\n')
    with pytest.raises(NotImplementedError, match="skeletons_file"):
        run_evaluation(str(cfg), "gt")
    cfg.write_text(f'seg_datasets = ["{tmp_path}/v.zarr/seg"]\n[pred]\npred_dataset = "{tmp_path}/v.zarr/pred/raw"\n')
    with pytest.raises(ValueError, match="Unknown type"):
        run_evaluation(str(cfg), "pred")
    assert not os.path.exists(tmp_path / "results_pred_v.json") and not os.path.exists(tmp_path / "results_gt_v.json")


def test_input_validation_messages(tmp_path):
    from bootstrapper_amd.evaluate import compute_errors
    store = str(tmp_path / "v.zarr")
    seg = _ds(store + "/seg", np.ones((4, 5, 6), np.uint64))
    _ds(store + "/p8/3d_affs", np.zeros((6, 4, 5, 6), np.uint8))
    _ds(store + "/pf/3d_affs", np.zeros((3, 4, 5, 6), np.float32))
    _ds(store + "/vs/3d_affs", np.zeros((3, 4, 5, 6), np.uint8), voxel_size=(2, 1, 1))
    outs = [(store + "/o/error_map", store + "/o/error_mask")]
    with pytest.raises(ValueError, match="3 offsets.*6 channels"):
        compute_errors([seg.path], store + "/p8/3d_affs", None, outs, aff_neighborhood=[[1, 0, 0], [0, 1, 0], [0, 0, 1]], engine="unused")
    with pytest.raises(ValueError, match="must be uint8"):
        compute_errors([seg.path], store + "/pf/3d_affs", None, outs, engine="unused")
    with pytest.raises(ValueError, match="voxel sizes differ"):
        compute_errors([seg.path], store + "/vs/3d_affs", None, outs, engine="unused")
    assert not os.path.exists(store + "/o")


def test_seg_to_affgraph_both_signs():
    seg = np.array([[[1, 1, 2, 0, 3, 3]]], np.uint64)
    pos = R.seg_to_affgraph(seg, [[0, 0, 1]])[0, 0, 0]
    neg = R.seg_to_affgraph(seg, [[0, 0, -1]])[0, 0, 0]
    assert pos.tolist() == [1, 0, 0, 0, 1, 0]     # seg[x] == seg[x + 1], both non-zero; the last voxel has no neighbour
    assert neg.tolist() == [0, 1, 0, 0, 0, 1]     # seg[x] == seg[x - 1]
    far = R.seg_to_affgraph(np.array([[[5], [5], [5]]], np.uint64), [[0, 2, 0], [0, -2, 0]])
    assert far[0, 0, :, 0].tolist() == [1, 0, 0] and far[1, 0, :, 0].tolist() == [0, 0, 1]


def test_scan_chunk_placement():
    from bootstrapper_amd.evaluate import scan_origins
    assert R.scan_origins(23, 10) == scan_origins(23, 10) == [0, 10, 13]
    assert R.scan_origins(50, 32) == scan_origins(50, 32) == [0, 18]
    assert R.scan_origins(64, 32) == [0, 32] and R.scan_origins(7, 10) == [0] and R.scan_origins(10, 10) == [0]
    order = R.scan_chunks((23, 50, 61), (10, 32, 32))
    assert order[:4] == [(0, 0, 0), (10, 0, 0), (13, 0, 0), (0, 18, 0)] and order[-1] == (13, 18, 29) and len(order) == 12


def test_aff_errors_last_chunk_wins_on_overlap():
    """a voxel covered by two chunks is normalised by the later chunk's maximum"""
    seg = np.ones((1, 1, 5), np.uint64)
    pred = np.array([[[[0, 255, 200, 128, 0]]]], np.uint8)   # x = 4: no neighbour inside the dataset, s = 0 = p
    emap, emask = R.aff_errors(seg, (0, 0, 0), pred, [[0, 0, 1]], (1, 1, 3))
    f = np.float32
    diff = [(f(1) - f(v) * f(1 / 255)) ** 2 for v in (0, 255, 200, 128)] + [f(0)]
    # chunks [0, 3) and [2, 5): x = 2 belongs to the second, whose maximum is x = 3's
    want = [diff[0] / diff[0], diff[1] / diff[0], diff[2] / diff[3], diff[3] / diff[3], f(0)]
    assert emap[0, 0].tolist() == [int(f(w) * f(255)) for w in want]
    assert emap[0, 0, 2] != int(diff[2] / diff[0] * f(255))
    assert emask[0, 0].tolist() == [int(f(0.1) < w < f(1.0)) for w in want]


def test_rand_voi_closed_forms():
    from bootstrapper_amd.evaluate import merge_pairs, rand_voi_from_table
    gt = np.array([1, 1, 2, 2], np.uint64)
    cases = {
        "identical": (gt, np.array([7, 7, 9, 9], np.uint64), dict(rand_split=1, rand_merge=1, voi_split=0, voi_merge=0)),
        "split": (np.array([1, 1, 1, 1], np.uint64), np.array([3, 3, 4, 4], np.uint64),
                  dict(rand_split=0.5, rand_merge=1, voi_split=1, voi_merge=0, nvi_split=1, nvi_merge=0)),
        "merge": (gt, np.array([0, 0, 0, 0], np.uint64), dict(rand_split=1, rand_merge=0.5, voi_split=0, voi_merge=1, nvi_merge=1)),
    }
    for name, (g, s, want) in cases.items():
        for got in (R.rand_voi(g, s), rand_voi_from_table(*merge_pairs([R.contingency(g, s)]))):
            for k, v in want.items():
                assert got[k] == pytest.approx(v, abs=1e-15), (name, k, got)
    # gt 0 is ignored wherever it is
    g0 = np.array([0, 1, 1, 0, 2, 2, 0], np.uint64)
    s0 = np.array([5, 7, 7, 6, 9, 9, 7], np.uint64)
    assert R.rand_voi(g0, s0) == R.rand_voi(gt, np.array([7, 7, 9, 9], np.uint64))
    # the mask multiplies both ids
    m = np.array([1, 1, 0, 2], np.uint8)
    assert [x.tolist() for x in R.contingency(gt, np.array([3, 4, 5, 6], np.uint64), m)] == [[1, 1, 4], [3, 4, 12], [1, 1, 1]]


def test_merge_pairs_sums_exactly_across_tiles():
    from bootstrapper_amd.evaluate import merge_pairs
    big = np.uint64(2**64 - 2)
    a = (np.array([big, 1], np.uint64), np.array([0, 2**40], np.uint64), np.array([2**60, 3], np.uint64))
    b = (np.array([1, big], np.uint64), np.array([2**40, 0], np.uint64), np.array([5, 2**60 + 1], np.uint64))
    g, s, n = merge_pairs([a, b])
    assert g.tolist() == [1, 2**64 - 2] and s.tolist() == [2**40, 0] and n.tolist() == [8, 2**61 + 1]


def test_stats_from_histogram_match_compute_stats():
    from bootstrapper_amd.evaluate import stats_from_histogram
    rng = np.random.default_rng(5)
    for a in (rng.integers(0, 256, (7, 9, 11), dtype=np.uint8), np.zeros((3, 4, 5), np.uint8),
              (rng.random((5, 6, 7)) < 0.3).astype(np.uint8)):
        ref = R.compute_stats(a)
        got = stats_from_histogram(np.bincount(a.ravel(), minlength=256))
        assert got["mean"] == ref["mean"] and got["num_nonzero_voxels"] == ref["num_nonzero_voxels"]
        assert got["total_voxels"] == ref["total_voxels"] and got["nonzero_ratio"] == ref["nonzero_ratio"]
        assert abs(got["std"] - ref["std"]) <= 1e-12 * max(1.0, ref["std"])
        json.dumps(got)
