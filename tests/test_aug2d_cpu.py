"""Host side of the geometric augmentation of the 2-D setups (bootstrapper_amd/augment2d.py) and the numpy restatement the
GPU tests compare against (tests/aug2d_ref.py): the restatement against scipy, the plan's bound, the draw order, the TOML
key and its refusals, the packed descriptor table, and -- on a float32 emulation of the kernels reading that table -- that
the comparisons of tests/test_aug2d_gpu.py catch the faults such batched kernels are prone to.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug2d_ref as R  # noqa: E402
import aug_ref  # noqa: E402
from bootstrapper_amd import augment2d as A  # noqa: E402

VS = (40, 4, 4)
FRAME = ((-2, -2), (26, 26))   # input (24, 24), output (16, 16), label margins 6


def drawn_plans(n, seed, K=3):
    rng = np.random.default_rng(seed)
    params = A.Aug2DParams(deform_p=1.0, control_point_spacing=(32, 32))   # nodes every 8 pixels: several cells in a small frame
    return [A.draw_plan2d(rng, params, (24, 24), FRAME, K, VS) for _ in range(n)]


def test_reference_bilinear_matches_scipy():
    from scipy.ndimage import map_coordinates
    rng = np.random.default_rng(0)
    crop = rng.integers(0, 256, (19, 23), dtype=np.uint8)
    s = np.stack([rng.uniform(0, n - 1, (9, 11)) for n in crop.shape]).astype(np.float32)
    want = map_coordinates(crop.astype(np.float64), s.astype(np.float64), order=1)
    assert np.abs(R.bilinear_f64(s, crop) - want).max() < 1e-10
    # ... and through the map of drawn plans: every pixel of the frame, every section
    for plan in drawn_plans(3, seed=1):
        lo, hi = A.source_box2d(plan)
        crop = rng.integers(0, 256, (plan.sections, hi[0] - lo[0], hi[1] - lo[1]), dtype=np.uint8)
        coords = R.map_f64(plan, lo).astype(np.float32)
        got = R.ref_raw(coords[None], [plan], [crop])
        for k in range(plan.sections):
            ks = plan.sections - 1 - k if plan.mirror[0] else k
            want = map_coordinates(crop[ks].astype(np.float64), coords[k].astype(np.float64), order=1) * 2 / 255 - 1
            assert np.abs(got[k, 0] - want).max() < 1e-12


def test_reference_nearest_matches_scipy_away_from_ties():
    """order 0 leaves out the pixels whose coordinate lies within 1e-6 of a half-integer: at most 1 % of them"""
    from scipy.ndimage import map_coordinates
    rng = np.random.default_rng(2)
    for plan in drawn_plans(4, seed=3):
        lo, hi = A.source_box2d(plan)
        crop = rng.integers(1, 2 ** 40, (hi[0] - lo[0], hi[1] - lo[1]), dtype=np.int64)
        coords = R.map_f64(plan, lo).astype(np.float32)
        s = coords[plan.sections // 2]
        frac = s - np.floor(s)
        away = (np.abs(frac - 0.5) > 1e-6).all(axis=0)
        assert 1.0 - away.mean() <= 0.01, away.mean()
        # scipy interpolates in float64, so the ids go through an index plane instead
        index = np.arange(crop.size, dtype=np.float64).reshape(crop.shape)
        want = crop.ravel()[map_coordinates(index, s.astype(np.float64), order=0).astype(np.int64)]
        assert np.array_equal(R.ref_nearest(coords[None], [plan], [crop])[0][away], want[away])


def test_nearest_rule_is_float32_floor_of_s_plus_half():
    crop = np.arange(3 * 8, dtype=np.int64).reshape(3, 8)
    s = np.zeros((2, 1, 4), dtype=np.float32)
    s[1, 0] = [2.5, np.nextafter(np.float32(2.5), np.float32(0)), 3.4999998, -3.0]   # tie goes up; one ulp below stays; clamp
    assert R.sample_nearest(s, crop)[0].tolist() == [3, 2, 3, 0]


def test_source_box_contains_the_map_for_50_drawn_plans():
    rng = np.random.default_rng(5)
    params = A.Aug2DParams(deform_p=1.0)
    for k in range(50):
        i, o = int(rng.integers(12, 40)) * 2, int(rng.integers(3, 6)) * 2
        margin = int(rng.integers(0, 2 * i))   # a labels window smaller and larger than the input section
        frame = A.frame_of((i, i), (o, o), (margin, margin), (margin, 0))
        plan = A.draw_plan2d(rng, params, (i, i), frame, int(rng.integers(1, 5)), VS)
        lo, hi = A.source_box2d(plan)
        assert R.box_contains(lo, hi, R.map_f64(plan, lo)), (k, i, frame)
        # a region: the input section; its box is no larger and contains the map there
        region = ((0, 0), (i, i))
        rlo, rhi = A.source_box2d(plan, region)
        s = R.map_f64(plan, rlo)[:, :, -frame[0][0]:-frame[0][0] + i, -frame[0][1]:-frame[0][1] + i]
        assert R.box_contains(rlo, rhi, s)
        assert all(a >= b for a, b in zip(rlo, lo)) and all(a <= b for a, b in zip(rhi, hi))


def test_frame_and_lattice_follow_the_rule():
    # the shipped 2d_mtlsd shape: input 196, output 104, LSD context 60 at a 4 nm grid against a network context of 46
    frame = A.frame_of((196, 196), (104, 104), (60, 60), (60, 60))
    assert frame == ((-14, -14), (210, 210))
    assert A.lattice_shape(frame, (40.0, 40.0)) == (9, 9)      # node j at -14 + (j - 1) 40: j = 0 .. ceil(223 / 40) + 2
    assert A.frame_of((17, 33), (9, 25), (2, 0), (0, 2)) == ((0, 0), (17, 33))     # labels inside the input: the frame is the input
    assert A.frame_of((24, 24), (16, 16), (6, 6), (6, 6)) == FRAME
    lo, hi = A.source_box2d(A.Aug2DPlan((24, 24), FRAME, 3))
    assert lo == (-3, -3) and hi == (28, 28)                   # identity: the frame plus the margin


def test_draw_plan_order_is_deterministic_and_draws_nothing_when_off():
    p = A.Aug2DParams(deform_p=1.0)
    a, b = (A.draw_plan2d(np.random.default_rng(9), p, (24, 24), FRAME, 3, VS) for _ in range(2))
    assert a.mirror == b.mirror and a.swap == b.swap and a.u == b.u and a.theta == b.theta
    assert np.array_equal(a.lattice, b.lattice) and np.array_equal(a.shifts, b.shifts) and np.array_equal(a.linear, b.linear)
    assert a.lattice.dtype == np.float32 and a.shifts.dtype == np.int32 and a.shifts.shape == (2, 3)
    # reference arguments at voxel size (40, 4, 4): nodes every 40 pixels, sigma 2 pixels; 2 components, no z
    assert a.lattice.shape == (2,) + A.lattice_shape(FRAME, (40.0, 40.0)) == (2, 4, 4)
    assert np.allclose(a.inv_spacing, [1 / 40, 1 / 40]) and 0.9 <= a.u <= 1.1 and 0 <= a.theta < 2 * np.pi
    # the order, replayed by hand: 4 flags; applied?, u, theta, lattice; applied?, step mask, steps, slip mask, slips
    rng = np.random.default_rng(9)
    flags = [bool(rng.random() < 0.5) for _ in range(4)]
    assert (a.mirror, a.swap) == (tuple(flags[:3]), flags[3])
    assert rng.random() < 1.0
    assert a.u == float(rng.uniform(0.9, 1.1)) and a.theta == float(rng.uniform(0, 2 * np.pi))
    assert np.array_equal(a.lattice, (rng.standard_normal((2, 4, 4)) * 2.0).astype(np.float32))
    assert rng.random() < 1.0                                   # shift_p = 1.0 still takes its draw
    on, step = rng.random(3) < 0.2, np.rint(rng.normal(0, 3.0, (3, 2)))
    slip_on, slip = rng.random(3) < 0.2, np.rint(rng.normal(0, 3.0, (3, 2)))
    assert np.array_equal(a.shifts, (np.cumsum(step * on[:, None], axis=0) + slip * slip_on[:, None]).T.astype(np.int32))
    after = rng.bit_generator.state
    rng2 = np.random.default_rng(9)
    A.draw_plan2d(rng2, p, (24, 24), FRAME, 3, VS)
    assert rng2.bit_generator.state == after                    # nothing else is drawn
    # ShiftAugment is drawn only when adj_slices > 1
    rng = np.random.default_rng(3)
    one = A.draw_plan2d(rng, A.Aug2DParams(simple=False, deform_p=0.0), (24, 24), FRAME, 1, VS)
    assert one.shifts is None and rng.bit_generator.state == np.random.default_rng(3).bit_generator.state
    off = A.draw_plan2d(rng, A.Aug2DParams(simple=False, deform_p=0.0, shift_p=0.0), (24, 24), FRAME, 3, VS)
    assert rng.bit_generator.state == np.random.default_rng(3).bit_generator.state
    assert off.mirror == (False, False, False) and not off.swap and off.lattice is None and off.shifts is None
    assert off.linear.tolist() == [1, 0, 0, 1]


def test_refusals_of_the_plan():
    with pytest.raises(ValueError, match="square"):
        A.draw_plan2d(np.random.default_rng(0), A.Aug2DParams(), (16, 20), ((0, 0), (16, 20)), 3, VS)
    with pytest.raises(NotImplementedError, match="voxel_size"):
        A.draw_plan2d(np.random.default_rng(0), A.Aug2DParams(simple=False, deform_p=1.0), (16, 16), ((0, 0), (16, 16)), 3, (40, 4, 8))
    A.draw_plan2d(np.random.default_rng(0), A.Aug2DParams(simple=False, deform_p=1.0, rotate=False), (16, 20), ((0, 0), (16, 20)), 3, (40, 4, 8))
    with pytest.raises(ValueError, match="at most 4096"):
        A.draw_plan2d(np.random.default_rng(0), A.Aug2DParams(deform_p=1.0, control_point_spacing=(4, 4)), (96, 96), ((0, 0), (96, 96)), 3, VS)


def test_toml_key_parsing():
    assert A.Aug2DParams.from_config(None) is None and A.Aug2DParams.from_config(False) is None
    d = A.Aug2DParams.from_config(True)
    assert (d.simple, d.deform_p, d.scale_interval, d.rotate, d.shift_p, d.prob_slip, d.prob_shift, d.shift_sigma) == \
        (True, 0.5, (0.9, 1.1), True, 1.0, 0.2, 0.2, 3.0)
    assert d.control_point_spacing is None and d.jitter_sigma is None
    p = A.Aug2DParams.from_config({"deform_p": 1, "scale_interval": [0.8, 1.2], "rotate": False, "control_point_spacing": [80, 80],
                                   "jitter_sigma": [8, 8], "shift_p": 0.25, "prob_slip": 0.1, "prob_shift": 0.3, "shift_sigma": 2, "simple": False})
    assert p == A.Aug2DParams(False, 1.0, (0.8, 1.2), False, (80.0, 80.0), (8.0, 8.0), 0.25, 0.1, 0.3, 2.0)
    with pytest.raises(ValueError, match="unknown augment2d key.*subsample"):
        A.Aug2DParams.from_config({"subsample": 4})
    with pytest.raises(ValueError, match="two world-unit values"):
        A.Aug2DParams.from_config({"control_point_spacing": [40, 40, 40]})
    with pytest.raises(ValueError, match="probability"):
        A.Aug2DParams.from_config({"deform_p": 1.5})
    with pytest.raises(ValueError, match="augment2d must be"):
        A.Aug2DParams.from_config("yes")


TWO_D = {"input_shape": [64, 64], "output_shape": [32, 32], "downsample_factors": [[2, 2]],
         "outputs": {"2d_affs": {"dims": 2, "neighborhood": [[-1, 0], [0, -1]]}}}
NHOOD3 = [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]


def test_make_sample_source_refuses_the_key_where_it_is_not_built():
    from bootstrapper_amd.train import make_sample_source
    first = {"input_shape": [8, 32, 32], "output_shape": [4, 16, 16], "outputs": {"3d_affs": {"dims": 3, "neighborhood": NHOOD3}}}
    with pytest.raises(NotImplementedError, match="augment2d.*3d_affs"):
        make_sample_source({"samples": [], "augment2d": True}, first)
    second = {"input_shape": [8, 32, 32], "output_shape": [4, 16, 16], "inputs": {"3d_lsds": {"sigma": 8}},
              "outputs": {"3d_affs": {"dims": 3, "neighborhood": NHOOD3}}}
    with pytest.raises(NotImplementedError, match="augment2d.*3d_affs_from_3d_lsd"):
        make_sample_source({"synthetic_labels": True, "augment2d": {"deform_p": 0.3}}, second)
    with pytest.raises(ValueError, match="unknown augment2d key.*jitter"):
        make_sample_source({"samples": [], "augment2d": {"jitter": 2}}, TWO_D)
    # `augment` with a 2-D setup stays refused, and now names the key that is built
    with pytest.raises(NotImplementedError, match="2-D setups.*augment2d"):
        make_sample_source({"samples": [], "augment": True}, TWO_D)


def test_section_source_refuses_before_any_read():
    from bootstrapper_amd.train import SectionSource
    affs = {"dims": 2, "neighborhood": [[-1, 0], [0, -1]]}
    with pytest.raises(ValueError, match="square"):
        SectionSource([], (48, 40), (32, 24), affs=affs, augment=True)
    with pytest.raises(ValueError, match="must be even"):
        SectionSource([], (48, 48), (33, 33), affs=affs, augment=True)


def test_without_the_key_no_plan_is_drawn(tmp_path, monkeypatch):
    """make_sample_source without `augment2d` builds a source with augment None, whose batches take the un-augmented path:
    draw_plan2d is not reachable from it"""
    from bootstrapper_amd import train as T
    from bootstrapper_amd.zarr_io import prepare_ds
    store = str(tmp_path / "vol.zarr")
    for name, dtype in (("raw", np.uint8), ("labels", np.uint64)):
        prepare_ds(f"{store}/{name}", (4, 80, 80), offset=(0, 0, 0), voxel_size=VS, chunk_shape=(4, 80, 80), dtype=dtype)
    cfg = {"samples": [{"raw": f"{store}/raw", "labels": f"{store}/labels"}]}
    monkeypatch.setattr(A, "draw_plan2d", lambda *a, **k: pytest.fail("draw_plan2d called without the key"))
    for value in (None, False):
        src = T.make_sample_source(dict(cfg, augment2d=value) if value is not None else cfg, TWO_D)
        assert isinstance(src, T.SectionSource) and src.augment is None
    class PlainPath(Exception):
        pass

    def plain_draw(self):   # the un-augmented path begins with its own location draws
        raise PlainPath
    called = []
    monkeypatch.setattr(T.SectionSource, "_next_augmented", lambda self: called.append(1))
    monkeypatch.setattr(T.SectionSource, "_draw", plain_draw)
    with pytest.raises(PlainPath):
        next(src)
    assert not called
    on = T.make_sample_source(dict(cfg, augment2d=True), TWO_D)
    assert on.augment == A.Aug2DParams() and on.frame == ((0, 0), (64, 64))
    next(on)
    assert called


def test_packed_table_holds_the_plans():
    plans, boxes, _ = R.build_case("24sq_K3", 4.0)
    p = A.Packed2D(plans, boxes)
    assert (p.S, p.K, p.shape, p.frame_shape) == (3, 3, (24, 24), (28, 28))
    import ctypes
    assert ctypes.sizeof(p.draws) == 3 * 64
    assert [d.flags for d in p.draws] == [1 | 4 | 8, 0, 2]
    assert list(p.draws[1].n) == [0, 0] and list(p.draws[0].n) == list(plans[0].lattice.shape[1:])
    assert p.draws[2].lattice_offset == plans[0].lattice.size and p.lattice.size == plans[0].lattice.size + plans[2].lattice.size
    assert len(set(p.crop_shapes)) == 3                                       # the crops differ in shape
    assert p.crop_offsets == [0, p.crop_shapes[0][0] * p.crop_shapes[0][1], sum(h * w for h, w in p.crop_shapes[:2])]
    assert p.shifts.shape == (3, 2, 3) and not p.shifts[1].any() and np.array_equal(p.shifts[2], plans[2].shifts)
    assert [round(v, 3) for v in p.draws[1].src] == [11.5 - boxes[1][0][0], 11.5 - boxes[1][0][1]]
    raw, lab, _ = R.build_crops(boxes, 3)
    flat = p.pack(raw, np.uint8)
    assert flat.size == 3 * p.crop_pixels
    h, w = p.crop_shapes[1]
    assert np.array_equal(flat[3 * p.crop_offsets[1]:3 * (p.crop_offsets[1] + h * w)].reshape(3, h, w), raw[1])
    with pytest.raises(ValueError, match="crop 0"):
        p.pack(lab[::-1], np.int64)


def emulated(case, spacing, fault=None):
    plans, boxes, window = R.build_case(case, R.SPACINGS[spacing])
    crops = R.build_crops(boxes, plans[0].sections)
    p = A.Packed2D(plans, boxes)
    packed = [p.pack(c, c[0].dtype) for c in crops]
    coords = R.emulate_coords(plans, boxes, fault)
    outputs = [(R.emulate_raw(coords, plans, packed[0], p.crop_shapes, p.crop_offsets, region, fault),
                R.emulate_nearest(coords, plans, packed[1], p.crop_shapes, p.crop_offsets, region, fault),
                R.emulate_nearest(coords, plans, packed[2], p.crop_shapes, p.crop_offsets, region, fault)) for region in R.regions(plans, window)]
    return plans, R.compare(plans, boxes, crops, window, coords, outputs)


@pytest.mark.parametrize("case", sorted(R.CASES))
@pytest.mark.parametrize("spacing", sorted(R.SPACINGS))
def test_emulated_kernels_pass_the_derived_gates(case, spacing):
    """float32 numpy, no fused multiply-add: the gates of the GPU test hold for the arithmetic they were derived for"""
    plans, res = emulated(case, spacing)
    assert R.passes(res), res
    assert len({(p.mirror, p.swap, p.u) for p in plans}) == 3 and plans[1].lattice is None and plans[1].shifts is None
    full = plans[0]
    if spacing == "spacing4":   # the case is what it claims: r leaves the lattice on both sides
        n, q = full.lattice.shape[1:], full.frame_shape
        assert (q[0] - 1 + full.shifts[0].max()) / 4.0 + 1 > n[0] - 1 and full.shifts[1].min() / 4.0 + 1 < 0
    else:
        assert full.lattice.shape[1:] == (4, 4)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_injected_faults_are_caught(fault):
    """each fault of a batched kernel, injected into the emulation, fails the comparison the GPU test makes"""
    _, res = emulated("24sq_K3", "spacing4", fault)
    assert not R.passes(res), (fault, res)
    # ... by the check it belongs to: the planes for the map's faults, the bit-equal labels / the raw gate for the sampling's
    if fault in ("previous_descriptor", "lattice_from_input_origin"):
        assert res["coords_excess"] > 1.0
    elif fault == "z_mirror_ignored":
        assert res["coords_excess"] <= 1.0 and res["labels_equal"] and res["raw_err"] > R.RAW_GATE
    elif fault == "labels_shift_of_section_0":
        assert res["coords_excess"] <= 1.0 and not res["labels_equal"] and not res["mask_equal"] and res["raw_err"] <= R.RAW_GATE
    else:
        assert res["coords_excess"] <= 1.0 and not res["labels_equal"] and res["raw_err"] > R.RAW_GATE


def test_exact_cases_of_the_reference():
    """identity, mirror, z-mirror, swap and integer shifts are numpy slices, flips and transposes of the crop (the same
    statements tests/test_aug2d_gpu.py makes about the device)"""
    lo = (-8, -8)
    rng = np.random.default_rng(3)
    lab, raw = rng.integers(1, 2 ** 40, (40, 40), dtype=np.int64), rng.integers(0, 256, (3, 40, 40), dtype=np.uint8)
    centre = lab[8:32, 8:32]

    def labels(plan):
        return R.ref_nearest(R.map_f64(plan, lo).astype(np.float32)[None], [plan], [lab], ((0, 0), (24, 24)))[0]
    assert np.array_equal(labels(A.Aug2DPlan((24, 24), FRAME, 3)), centre)
    assert np.array_equal(labels(A.Aug2DPlan((24, 24), FRAME, 3, mirror=(False, True, True))), centre[::-1, ::-1])
    assert np.array_equal(labels(A.Aug2DPlan((24, 24), FRAME, 3, swap=True)), centre.T)
    zm = A.Aug2DPlan((24, 24), FRAME, 3, mirror=(True, False, False))
    got = R.ref_raw(R.map_f64(zm, lo).astype(np.float32)[None], [zm], [raw], ((0, 0), (24, 24)))[:, 0]
    assert np.abs(got - (raw[::-1, 8:32, 8:32] * 2.0 / 255.0 - 1.0)).max() < 1e-12
    assert np.array_equal(labels(zm), centre)


def test_alignment_condition_is_met_by_the_reference_alone():
    """tests/test_train2d_aug_gpu.py checks raw's centre channel against the label's value wherever the 3 x 3 neighbourhood of
    the augmented labels is uniform and non-zero, and requires those pixels to be at least 20 % of each batch.  Its store meets
    that for the batches it draws (same seed, same draw order, same rejection rounds) through aug2d_ref alone, and there raw is
    the label's value."""
    import test_train2d_aug_gpu as T
    raw, labels = aug_ref.boxes_volume(T.VOLUME, T.BOX)
    lo = hi = T.label_margins()
    shares = []
    for raw_b, lab_b in R.simulate_batches(raw, labels, A.Aug2DParams.from_config(T.ALIGN), T.INPUT, T.OUTPUT, lo, hi, T.ADJ, T.VOXEL_SIZE,
                                           T.BATCHES):
        share, err = R.alignment(raw_b, lab_b)
        assert err <= R.RAW_GATE
        shares.append(share)
    assert min(shares) >= 0.2, shares
