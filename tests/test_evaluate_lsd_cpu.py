"""LSD error maps of `bs evaluate`, host side: the restatement's morphology (tests/lsd_errors_ref.py), the opt-in and the
refusals, the default sigma and context, and the device kernel's formula against the oracle on thin objects.  No GPU."""
import os

import numpy as np
import pytest
from click.testing import CliRunner

import lsd_errors_cases as K
import lsd_errors_ref as L
from eval_ref import padded


def _ds(path, a, offset=(0, 0, 0), voxel_size=(1, 1, 1), chunk=None):
    from bootstrapper_amd.zarr_io import prepare_ds
    d = prepare_ds(path, a.shape, offset=offset, voxel_size=voxel_size, chunk_shape=chunk or a.shape, dtype=a.dtype,
                   axis_names=(["c^"] if a.ndim == 4 else []) + ["z", "y", "x"], units=["nm"] * 3)
    d[:] = a
    return d


def test_iterated_morphology_is_one_opening_and_one_closing():
    """binary_erosion / binary_dilation with the cross, iterations = 4, border_value = 0, equal one erosion and one dilation
    by the L1 diamond of radius 4; the z closing with border_value = 0 empties the array's first and last slice"""
    rng = np.random.default_rng(3)
    from scipy.ndimage import gaussian_filter
    for i in range(6):
        shape = [(7, 30, 33), (3, 21, 40), (12, 36, 36), (2, 25, 25), (5, 9, 50), (1, 20, 20)][i]
        a = gaussian_filter(rng.random(shape), (0.7, 2.5, 2.5)) > 0.5 - 0.02 * i
        a |= rng.random(shape) < 0.02
        got, one = L.morphology(a), L.morphology_one_pass(a)
        assert got.dtype == np.uint8 and np.array_equal(got, one), i
        assert not got[0].any() and not got[-1].any()
        if i in (0, 2):
            assert got.any() and (got != a).any()


def test_morphology_hand_cases():
    def run(fill):
        a = np.zeros((5, 30, 30), bool)
        fill(a)
        return L.morphology(a)
    sq9 = run(lambda a: a.__setitem__((slice(1, 4), slice(8, 17), slice(10, 19)), True))
    # the 9 x 9 square is eroded to its centre and dilated back to the diamond of radius 4 around it
    want = np.zeros((30, 30), np.uint8)
    want[8:17, 10:19] = L.diamond(4)[0]
    assert np.array_equal(sq9[2], want) and np.array_equal(sq9[1], want) and np.array_equal(sq9[3], want)
    assert not sq9[0].any() and not sq9[4].any()
    assert not run(lambda a: a.__setitem__((slice(1, 4), slice(8, 16), slice(10, 18)), True)).any()      # 8 x 8 vanishes
    assert not run(lambda a: a.__setitem__((slice(1, 4), slice(8, 16), slice(4, 26)), True)).any()       # a line 8 wide vanishes
    assert run(lambda a: a.__setitem__((slice(1, 4), slice(8, 17), slice(4, 26)), True))[2, 12, 8:22].all()   # 9 wide survives
    # the array's edge does not stand in for a missing row: the erosion reads 0 outside (8 rows at the edge vanish, 9 stay)
    assert not run(lambda a: a.__setitem__((slice(1, 4), slice(0, 8), slice(10, 19)), True)).any()
    assert not run(lambda a: a.__setitem__((slice(1, 4), slice(8, 17), slice(22, 30)), True)).any()
    assert run(lambda a: a.__setitem__((slice(1, 4), slice(0, 9), slice(21, 30)), True))[2, 0, 25]
    # a one-slice gap in z closes
    def gap(a):
        a[1, 8:17, 10:19] = True
        a[3, 8:17, 10:19] = True
    g = run(gap)
    assert np.array_equal(g[2], want) and np.array_equal(g[1], want) and np.array_equal(g[3], want)
    # so does a two-slice gap (both dilations meet); a three-slice gap stays open
    a = np.zeros((8, 30, 30), bool)
    a[[1, 4], 8:17, 10:19] = True
    assert all(np.array_equal(p, want) for p in L.morphology(a)[1:5])
    a = np.zeros((8, 30, 30), bool)
    a[[1, 5], 8:17, 10:19] = True
    g3 = L.morphology(a)
    assert g3[1].any() and g3[5].any() and not g3[2:5].any()


def test_default_sigma_and_context():
    from bootstrapper_amd.evaluate import LSD_DOWNSAMPLE, LSD_MARGIN, lsd_setup
    s = lsd_setup((40, 8, 8))
    assert s["sigma"] == [80, 80, 80] and s["context"] == [6, 30, 30] and s["margin"] == [2, 50, 50] == LSD_MARGIN
    assert s["downsample"] == 2 == LSD_DOWNSAMPLE == L.DOWNSAMPLE and tuple(LSD_MARGIN) == L.MARGIN
    assert L.default_sigma((40, 8, 8)) == 80 and L.context_voxels(80, (40, 8, 8)) == [6, 30, 30]
    s = lsd_setup((8, 8, 8), lsd_sigma=16, lsd_margin=[2, 6, 6])
    assert s["sigma"] == [16, 16, 16] and s["context"] == [6, 6, 6] and s["margin"] == [2, 6, 6]
    assert lsd_setup((50, 4, 4), lsd_sigma=70)["context"] == [4, 52, 52]      # 210 / 50 snapped by shrinking
    with pytest.raises(ValueError, match="lsd_sigma"):
        lsd_setup((8, 8, 8), lsd_sigma=[16, 16, 16])
    with pytest.raises(ValueError, match="lsd_margin"):
        lsd_setup((8, 8, 8), lsd_margin=[2, 6])


def test_help_lists_lsd_errors():
    from bootstrapper_amd.cli import cli
    for name in ("evaluate", "eval"):
        r = CliRunner().invoke(cli, [name, "--help"])
        assert r.exit_code == 0 and "--lsd_errors" in r.output, (name, r.output)


def test_opt_in_and_refusals(tmp_path):
    from bootstrapper_amd.evaluate import compute_errors, run_evaluation
    store = str(tmp_path / "v.zarr")
    vs = (40, 8, 8)
    seg = _ds(store + "/seg", np.ones((8, 24, 24), np.uint64), voxel_size=vs)
    _ds(store + "/ok/3d_lsds", np.zeros((10, 8, 24, 24), np.uint8), voxel_size=vs, chunk=(10, 8, 24, 24))
    _ds(store + "/f32/3d_lsds", np.zeros((10, 8, 24, 24), np.float32), voxel_size=vs)
    _ds(store + "/six/3d_lsds", np.zeros((6, 8, 24, 24), np.uint8), voxel_size=vs)
    _ds(store + "/odd/3d_lsds", np.zeros((10, 8, 24, 24), np.uint8), voxel_size=vs, chunk=(10, 8, 24, 23))
    outs = [(store + "/o/error_map", store + "/o/error_mask")]
    # without the opt-in: the old refusal, from the function and from the command
    with pytest.raises(NotImplementedError, match="3d_lsds error maps are not part of this engine"):
        compute_errors([seg.path], store + "/ok/3d_lsds", None, outs, engine="unused")
    cfg = tmp_path / "04_eval_v.toml"
    cfg.write_text(f'seg_datasets = ["{seg.path}"]\n[pred]\npred_dataset = "{store}/ok/3d_lsds"\n')
    with pytest.raises(NotImplementedError, match="3d_lsds error maps are not part of this engine"):
        run_evaluation(str(cfg), "pred")
    r = CliRunner().invoke(__import__("bootstrapper_amd.cli", fromlist=["cli"]).cli, ["eval", str(cfg), "-p"])
    assert r.exit_code != 0 and isinstance(r.exception, NotImplementedError)

    def refused(pred, match, **kw):
        with pytest.raises(ValueError, match=match):
            compute_errors([seg.path], store + pred, None, outs, engine="unused", lsd_errors=True, **kw)
    refused("/f32/3d_lsds", "must be uint8")
    refused("/six/3d_lsds", "10 channels")
    refused("/odd/3d_lsds", "chunk \\+ 2 \\* lsd_margin = 123 voxels along x is not a multiple of the downsample factor 2")
    refused("/ok/3d_lsds", "chunk \\+ 2 \\* lsd_margin = 11 voxels along z", roi_offset=(0, 0, 0), roi_shape=(7 * 40, 24 * 8, 24 * 8))
    refused("/ok/3d_lsds", "context floor\\(3 \\* sigma / voxel_size\\) = 3 voxels along z", lsd_sigma=40)
    refused("/ok/3d_lsds", "window radius \\[6, 30, 30\\].*above the kernel's limit", lsd_sigma=160)
    assert not os.path.exists(store + "/o")
    assert not os.path.exists(tmp_path / "results_pred_v.json")


def test_kernel_formula_on_thin_objects():
    """the device kernel's formula (relative coordinates, a direct float64 sum; lsd_errors_ref.direct_descriptor) stays within
    1e-5 of the oracle on the one-voxel objects and the one-voxel-thick sheets, also where no tap of the window holds the
    label: so the GPU test keeps these objects under its 1e-4 gate"""
    vs, sigma, df, margin, ctx = (40, 8, 8), 80, 2, (2, 6, 6), (6, 30, 30)
    c = K.make_case(21, vs, sigma, df, (10, 40, 44), margin, ctx)
    chunk = (8, 24, 24)
    grown = [n + 2 * m for n, m in zip(chunk, margin)]
    from oracle.lsd_ref import lsd_targets
    worst, seen, empty = 0.0, {k: 0 for k in c["thin"]}, 0
    for org in ((0, 0, 0), (2, 16, 20)):
        begin = [b + o - m - k for b, o, m, k in zip(c["seg_begin"], org, margin, ctx)]
        labels = padded(c["seg"], begin, [g + 2 * k for g, k in zip(grown, ctx)])
        ref = lsd_targets(labels, ctx, grown, [float(sigma)] * 3, vs, df)[0]
        for name, vox in c["thin"].items():
            for v in vox:
                p = [int(x - b) for x, b in zip(v, begin)]
                g = [x - k for x, k in zip(p, ctx)]
                if not all(0 <= x < n for x, n in zip(g, grown)):
                    continue
                d = L.direct_descriptor(labels, p, [float(sigma)] * 3, vs, df)
                worst = max(worst, float(np.abs(d - ref[(slice(None),) + tuple(g)]).max()))
                seen[name] += 1
                empty += d[9] == 0
    print("thin objects: voxels compared", seen, "windows without a tap", empty, "worst |direct - oracle|", worst)
    assert min(seen.values()) > 0 and empty > 0
    assert worst < 1e-5
