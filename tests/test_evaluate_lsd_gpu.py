"""LSD error maps of `bs evaluate` on the MI355X (bsmi_eval_lsd_errors_u8): every stage against a reference run on that stage's
own inputs (the descriptors against oracle/lsd_ref.py to 1e-4, every later stage bit-equal to numpy / scipy on the device's own
previous output), the whole chain against tests/lsd_errors_ref.py within the bound the descriptor gate implies, and the driver
on an on-disk store."""
import json

import numpy as np
import pytest

import lsd_errors_cases as K
import lsd_errors_ref as L
from eval_ref import compute_stats, padded, scan_chunks, scan_origins

pytestmark = pytest.mark.gpu

E = 1e-4                       # the descriptor gate (the one bsmi_train_lsd_targets meets against the same oracle)
THRESHOLDS = (0.01, 0.5)       # pred pads with zeros inside the grown regions, whose diff of ~4 sets the maximum: the mismatch
                               # between the two segmentations sits at a few percent of it
CHUNK = (8, 24, 24)
SETTINGS = {
    # sub-grid radii (3, 15, 15); ROI (10, 40, 44): snapped last chunks on all axes, 8 chunks
    "aniso": dict(voxel_size=(40, 8, 8), sigma=80, downsample=2, context=(6, 30, 30), margin=(2, 6, 6), roi_shape=(10, 40, 44)),
    "aniso-nomask": dict(voxel_size=(40, 8, 8), sigma=80, downsample=2, context=(6, 30, 30), margin=(2, 6, 6), roi_shape=(10, 40, 44),
                         with_mask=False),
    "iso-df1": dict(voxel_size=(8, 8, 8), sigma=16, downsample=1, context=(6, 6, 6), margin=(2, 6, 6), roi_shape=(10, 40, 44)),
    "iso-df2": dict(voxel_size=(8, 8, 8), sigma=16, downsample=2, context=(6, 6, 6), margin=(2, 6, 6), roi_shape=(10, 40, 44)),
    # the reference's margin, two chunks
    "margin50": dict(voxel_size=(40, 8, 8), sigma=80, downsample=2, context=(6, 30, 30), margin=(2, 50, 50), roi_shape=(8, 24, 40)),
    # the bare chunk
    "margin0": dict(voxel_size=(40, 8, 8), sigma=80, downsample=2, context=(6, 30, 30), margin=(0, 0, 0), roi_shape=(10, 40, 44)),
}
_RUNS = {}


@pytest.fixture(scope="module")
def engine():
    from bootstrapper_amd.evaluate import EvalDevice
    e = EvalDevice(0)
    yield e
    e.close()


def chunk_index(roi_shape, chunk):
    """origin -> the device's chunk number (jz * ncy + jy) * ncx + jx"""
    oz, oy, ox = (scan_origins(n, c) for n, c in zip(roi_shape, chunk))
    return {(z, y, x): (iz * len(oy) + iy) * len(ox) + ix for iz, z in enumerate(oz) for iy, y in enumerate(oy) for ix, x in enumerate(ox)}


def device_run(eng, c, chunk=CHUNK, thresholds=THRESHOLDS, scratch_bytes=None):
    """the whole ROI as one tile, with the debug outputs"""
    torch = eng.torch
    T, m = c["roi_shape"], c["margin"]
    halo = [a + b for a, b in zip(m, c["context"])]
    seg_t = eng.to_dev(padded(c["seg"], [b - h for b, h in zip(c["seg_begin"], halo)], [t + 2 * h for t, h in zip(T, halo)]))
    grown = [t + 2 * a for t, a in zip(T, m)]
    pred_t = eng.to_dev(np.stack([padded(c["pred"][k], [b - a for b, a in zip(c["pred_begin"], m)], grown) for k in range(10)]))
    mask_t = None if c["mask"] is None else eng.to_dev(padded(c["mask"], [b - a for b, a in zip(c["mask_begin"], m)], grown))
    dbg = eng.lsd_debug_buffers(T, chunk, m)
    emap_t = torch.zeros(T, dtype=torch.uint8, device=eng.dev)
    emask_t = torch.full(T, 7, dtype=torch.uint8, device=eng.dev)
    hist_t = torch.zeros(257, dtype=torch.int64, device=eng.dev)
    lsd = {k: c[k] for k in ("margin", "context", "voxel_size", "downsample")}
    lsd["sigma"] = [c["sigma"]] * 3
    kw = {} if scratch_bytes is None else {"scratch_bytes": scratch_bytes}
    eng.lsd_errors(seg_t, [-h for h in halo], pred_t, mask_t, T, chunk, lsd, thresholds, T[0], emap_t, emask_t, hist_t, debug=dbg, **kw)
    eng.lib.check(eng.lib.lib.bsmi_eval_status(eng.h, eng.stream))
    out = {k: v.cpu().numpy() for k, v in dbg.items()}
    out.update(emap=emap_t.cpu().numpy(), emask=emask_t.cpu().numpy(), hist=hist_t.cpu().numpy())
    return out


def compose(c, desc, chunk=CHUNK, thresholds=THRESHOLDS):
    """numpy / scipy from given descriptors (per chunk over its grown region, device chunk order) to the outputs"""
    T, m = c["roi_shape"], c["margin"]
    chunk = [min(a, b) for a, b in zip(chunk, T)]
    grown = [a + 2 * b for a, b in zip(chunk, m)]
    index = chunk_index(T, chunk)
    emap, emask = np.zeros(T, np.uint8), np.zeros(T, np.uint8)
    crop = tuple(slice(a, a + n) for a, n in zip(m, chunk))
    for org in scan_chunks(T, chunk):
        g0 = [o - a for o, a in zip(org, m)]
        p = np.stack([padded(c["pred"][k], [b + g for b, g in zip(c["pred_begin"], g0)], grown) for k in range(10)])
        p = p.astype(np.float32) * np.float32(1.0 / 255)
        mk = None if c["mask"] is None else padded(c["mask"], [b + g for b, g in zip(c["mask_begin"], g0)], grown)
        d, _, _ = L.create_diff(desc[index[org]], p, mk)
        sl = tuple(slice(o, o + n) for o, n in zip(org, chunk))
        emask[sl] = L.morphology(L.threshold(d, thresholds))[crop]
        emap[sl] = (d[crop] * 255 + 0).astype(np.uint8)
    return emap, emask


def run_of(engine, name):
    """one case, one reference run and one device run per setting, shared by the tests below and left unchanged"""
    if name not in _RUNS:
        c = K.make_case(21, **SETTINGS[name])
        stages = []
        ref = L.lsd_errors(c["seg"], c["seg_begin"], c["pred"], c["pred_begin"], c["roi_shape"], CHUNK, c["sigma"], c["voxel_size"],
                           THRESHOLDS, c["mask"], c["mask_begin"], c["margin"], c["downsample"], stages)
        _RUNS[name] = (c, ref, stages, device_run(engine, c))
    return _RUNS[name]


@pytest.mark.parametrize("name", ["aniso", "iso-df1", "iso-df2", "margin50"])
def test_descriptors_against_the_oracle(engine, name):
    """check 1: max |device - oracle| < 1e-4 per channel, exactly 0 on background; the thin objects stay in (the kernel's
    formula is within 1e-5 of the oracle on them: test_evaluate_lsd_cpu.py::test_kernel_formula_on_thin_objects)"""
    c, _, stages, dev = run_of(engine, name)
    index = chunk_index(c["roi_shape"], CHUNK)
    m, ctx = c["margin"], c["context"]
    grown = [a + 2 * b for a, b in zip(CHUNK, m)]
    worst = np.zeros(10)
    thin_seen = big_seen = 0
    for st in stages:
        got = dev["desc"][index[st["origin"]]]
        assert got.shape == st["desc"].shape == (10,) + tuple(grown)
        worst = np.maximum(worst, np.abs(got - st["desc"]).max(axis=(1, 2, 3)))
        labels = padded(c["seg"], [b + o - a for b, o, a in zip(c["seg_begin"], st["origin"], m)], grown)
        assert np.all(got[:, labels == 0] == 0) and got[9][labels != 0].max() > 0
        thin_seen += int(np.isin(labels, list(K.THIN.values())).sum())
        big_seen += int((labels >= 2**32).sum())
    print(name, "max abs error per channel", worst)
    assert thin_seen > 0 and big_seen > 0
    assert worst.max() < E


@pytest.mark.parametrize("name", ["aniso", "aniso-nomask", "iso-df1", "iso-df2", "margin50", "margin0"])
def test_later_stages_bit_equal_on_the_device_s_own_outputs(engine, name):
    """check 2: diff from the device descriptors, the maxima, error_map and the raw mask from the device diff, the final mask
    from the device raw mask through scipy's iterated calls, histogram and statistics from the written outputs"""
    from bootstrapper_amd.evaluate import stats_from_histogram
    c, _, stages, dev = run_of(engine, name)
    T, m = c["roi_shape"], c["margin"]
    index = chunk_index(T, CHUNK)
    crop = tuple(slice(a, a + n) for a, n in zip(m, CHUNK))
    emap, emask = np.zeros(T, np.uint8), np.zeros(T, np.uint8)
    raws, finals = [], []
    for st in stages:   # Scan's order: the later chunk wins
        i = index[st["origin"]]
        g0 = [o - a for o, a in zip(st["origin"], m)]
        grown = st["diff"].shape
        mk = None if c["mask"] is None else padded(c["mask"], [b + g for b, g in zip(c["mask_begin"], g0)], grown)
        diff = np.sum((dev["desc"][i] - st["pred"]) ** 2, axis=0)
        if mk is not None:
            diff *= mk
        assert diff.dtype == np.float32 and np.array_equal(diff, dev["diff"][i]), (name, i, "diff")
        assert np.max(dev["diff"][i]) == dev["max"][i], (name, i, "max")
        d = dev["diff"][i] / dev["max"][i] if dev["max"][i] > 0 else np.zeros_like(dev["diff"][i])
        raw = L.threshold(d, THRESHOLDS)
        assert np.array_equal(raw.astype(np.uint8), dev["raw"][i]), (name, i, "raw mask")
        final = L.morphology(dev["raw"][i].astype(bool))
        raws.append(dev["raw"][i])
        finals.append(final)
        sl = tuple(slice(o, o + n) for o, n in zip(st["origin"], CHUNK))
        emap[sl] = (d[crop] * 255 + 0).astype(np.uint8)
        emask[sl] = final[crop]
    assert np.array_equal(dev["emap"], emap), int((dev["emap"] != emap).sum())
    assert np.array_equal(dev["emask"], emask), int((dev["emask"] != emask).sum())
    raws, finals = np.stack(raws), np.stack(finals)
    print(name, "raw mask ones", raws.mean(), "final mask ones", finals.mean(), "differ", (raws != finals).mean(), "error_mask", emask.mean())
    assert raws.any() and (raws != finals).any() and emap.any()       # no comparison above is vacuous
    if name == "margin0":   # the bare chunk: the z closing empties every chunk's first and last slice
        assert all(not f[0].any() and not f[-1].any() for f in finals) and not dev["emask"][0].any() and not dev["emask"][-1].any()
    else:
        assert finals.any() and (emask.any() or not name.startswith("aniso"))
    assert np.array_equal(dev["hist"][:256], np.bincount(dev["emap"].ravel(), minlength=256)) and dev["hist"][256] == int(dev["emask"].sum())
    total = int(np.prod(T))
    for got, ref in ((stats_from_histogram(dev["hist"][:256]), compute_stats(dev["emap"])),
                     (stats_from_histogram([total - int(dev["hist"][256]), int(dev["hist"][256])]), compute_stats(dev["emask"]))):
        assert got["mean"] == ref["mean"] and got["num_nonzero_voxels"] == ref["num_nonzero_voxels"]
        assert got["total_voxels"] == ref["total_voxels"] and abs(got["std"] - ref["std"]) <= 1e-12 * max(1.0, ref["std"])


@pytest.mark.parametrize("name", ["aniso", "aniso-nomask", "iso-df1", "iso-df2", "margin50"])
def test_whole_chain_against_the_restatement(engine, name):
    """check 3: with descriptors within E of the reference's a, (a' - p)^2 - (a - p)^2 = (a' - a)(a' + a - 2p) is at most
    2 E |a - p| + E^2 per channel; f32 rounding of ten terms of at most 1 adds less than 1e-6.  The mask is 0 or 1."""
    c, _, stages, dev = run_of(engine, name)
    index = chunk_index(c["roi_shape"], CHUNK)
    worst = 0.0
    for st in stages:
        bound = 2 * E * np.abs(st["desc"].astype(np.float64) - st["pred"]).sum(axis=0) + 10 * E * E + 1e-6
        err = np.abs(dev["diff"][index[st["origin"]]].astype(np.float64) - st["diff"])
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (name, st["origin"], float((err / bound).max()))
    print(name, "worst |diff_dev - diff_ref| / bound", worst)
    assert c["mask"] is None or int(c["mask"].max()) == 1


def test_chunk_groups_give_the_same_outputs(engine):
    """a scratch limit that holds two chunks at a time (8 chunks: four groups) changes nothing"""
    c, _, _, dev = run_of(engine, "aniso")
    grown, sub = 12 * 36 * 36, 12 * 48 * 48
    per_chunk = 4 * sub + 7 * grown
    small = device_run(engine, c, scratch_bytes=2 * per_chunk + 100)
    for k in ("emap", "emask", "hist", "desc", "diff", "max", "raw"):
        assert np.array_equal(small[k], dev[k]), k
    from bootstrapper_amd import _lib
    with pytest.raises(_lib.BsmiError, match="bytes of scratch"):
        device_run(engine, c, scratch_bytes=per_chunk - 1)


def _ds(path, a, offset, voxel_size, chunk):
    from bootstrapper_amd.zarr_io import prepare_ds
    d = prepare_ds(path, a.shape, offset=offset, voxel_size=voxel_size, chunk_shape=chunk, dtype=a.dtype,
                   axis_names=(["c^"] if a.ndim == 4 else []) + ["z", "y", "x"], units=["nm"] * 3)
    d[:] = a
    return d


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
def test_driver_on_a_store(tmp_path, engine, masked):
    """check 4: three segmentations (one over its own smaller ROI) against one 3d_lsds dataset through `run_evaluation` with
    the opt-in in the config; streamed layers and whole_roi = True give identical outputs, equal to the composition of the later
    stages (numpy / scipy) on the device's descriptors; JSON keys as in the affinity form; margin (0, 0, 0) reaches the kernel"""
    from bootstrapper_amd.evaluate import compute_errors, run_evaluation
    from bootstrapper_amd.zarr_io import open_ds
    vs = (40, 8, 8)
    s = dict(SETTINGS["aniso"], with_mask=masked)
    c = K.make_case(33, mask_max=2, **s)
    world = lambda v: [int(a) * b for a, b in zip(v, vs)]  # noqa: E731
    store = str(tmp_path / "vol.zarr")
    # world origin = the ROI's first voxel + (100, 100, 100) voxels
    at = lambda begin: world([100 - b for b in begin])  # noqa: E731
    seg_b = K.other_segmentation(c["seg"])
    small_begin, small_shape = (2, 8, 0), (8, 30, 44)       # the third segmentation's own ROI inside the ROI
    sl = tuple(slice(b + o, b + o + n) for b, o, n in zip(c["seg_begin"], small_begin, small_shape))
    seg_c = c["seg"][sl]
    segs = [_ds(store + "/segs/a", c["seg"], at(c["seg_begin"]), vs, (8, 32, 32)).path,
            _ds(store + "/segs/b", seg_b, at(c["seg_begin"]), vs, (8, 32, 32)).path,
            _ds(store + "/segs/c", seg_c, world([100 + o for o in small_begin]), vs, (8, 32, 32)).path]
    pred = _ds(store + "/pred/3d_lsds", c["pred"], at(c["pred_begin"]), vs, (10,) + CHUNK).path
    mask = _ds(store + "/mask", c["mask"], at(c["mask_begin"]), vs, (8, 32, 32)).path if masked else None
    cfg = tmp_path / "04_eval_vol.toml"
    cfg.write_text(f'''seg_datasets_prefix = "{store}/segs"
{f'mask_dataset = "{mask}"' if masked else ''}
[pred]
pred_dataset = "{pred}"
thresholds = [{THRESHOLDS[0]}, {THRESHOLDS[1]}]
lsd_errors = true
[pred.params]
lsd_margin = [2, 6, 6]
roi_offset = {world([100, 100, 100])}
roi_shape = {world(c["roi_shape"])}
''')
    run_evaluation(str(cfg), "pred")
    res = json.loads((tmp_path / "results_pred_vol.json").read_text())
    assert list(res) == segs
    # the same three through compute_errors as one tile each
    outs2 = [(store + f"/whole/{i}/error_map", store + f"/whole/{i}/error_mask") for i in range(3)]
    stats2 = compute_errors(segs, pred, mask, outs2, thresholds=THRESHOLDS, roi_offset=world([100, 100, 100]), roi_shape=world(c["roi_shape"]),
                            engine=engine, whole_roi=True, lsd_errors=True, lsd_margin=[2, 6, 6])
    engine.lib.check(engine.lib.lib.bsmi_eval_status(engine.h, engine.stream))
    for i, (sp, seg) in enumerate(zip(segs, (c["seg"], seg_b, None))):
        e = res[sp]
        assert list(e) == ["seg_ds", "pred_ds", "mask_ds", "map_ds", "thresholds", "error_map", "error_mask"]
        assert e["map_ds"] == sp + "__vs__3d_lsds/error_map" and e["mask_ds"] == sp + "__vs__3d_lsds/error_mask"
        assert e["pred_ds"] == pred and e["thresholds"] == list(THRESHOLDS)
        case = dict(c)
        if seg is None:   # the smaller ROI: zeros beyond the third dataset, pred and mask read on around it
            case.update(seg=seg_c, seg_begin=[0, 0, 0], roi_shape=list(small_shape),
                        pred_begin=[a + b for a, b in zip(c["pred_begin"], small_begin)],
                        mask_begin=[a + b for a, b in zip(c["mask_begin"], small_begin)])
        else:
            case["seg"] = seg
        dev = device_run(engine, case)
        want_map, want_mask = compose(case, dev["desc"])
        assert want_map.any() and want_mask.any()
        got_map, got_mask = open_ds(e["map_ds"]), open_ds(e["mask_ds"])
        off = world([100 + (small_begin[d] if seg is None else 0) for d in range(3)])
        assert got_map.dtype == np.uint8 and tuple(got_map.offset) == tuple(off) and tuple(got_map.voxel_size) == vs
        assert got_map.shape == tuple(case["roi_shape"]) and got_map.axis_names == ["z", "y", "x"]
        assert np.array_equal(got_map[:], want_map), (i, int((got_map[:] != want_map).sum()))
        assert np.array_equal(got_mask[:], want_mask), (i, int((got_mask[:] != want_mask).sum()))
        assert np.array_equal(open_ds(outs2[i][0])[:], want_map) and np.array_equal(open_ds(outs2[i][1])[:], want_mask)
        assert e["error_map"] == stats2[i][0] and e["error_mask"] == stats2[i][1]
        for key, ref in (("error_map", want_map), ("error_mask", want_mask)):
            st, rs = e[key], compute_stats(ref)
            assert st["mean"] == rs["mean"] and st["num_nonzero_voxels"] == rs["num_nonzero_voxels"]
            assert st["total_voxels"] == rs["total_voxels"] and abs(st["std"] - rs["std"]) <= 1e-12 * max(1.0, rs["std"])
    # margin (0, 0, 0): every chunk's first and last slice of error_mask is empty (z chunks [0, 8) and [2, 10))
    outs0 = [(store + "/bare/error_map", store + "/bare/error_mask")]
    compute_errors(segs[:1], pred, mask, outs0, thresholds=THRESHOLDS, roi_offset=world([100, 100, 100]), roi_shape=world(c["roi_shape"]),
                   engine=engine, lsd_errors=True, lsd_margin=[0, 0, 0])
    engine.lib.check(engine.lib.lib.bsmi_eval_status(engine.h, engine.stream))
    bare = open_ds(outs0[0][1])[:]
    assert not bare[0].any() and not bare[9].any() and not bare[2].any() and bare.any()
    assert not np.array_equal(bare, open_ds(res[segs[0]]["mask_ds"])[:])
