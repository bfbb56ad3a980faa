"""Host side of the geometric training augmentation (bootstrapper_amd/augment.py) and the numpy restatement the GPU tests
compare against (tests/aug_ref.py): the restatement against scipy, the plan's bound, the draw order, the TOML key and its
refusals, and -- on a float32 emulation of the kernels -- that the comparisons of tests/test_aug_gpu.py catch the faults
such kernels are prone to.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_ref as R  # noqa: E402
from bootstrapper_amd import augment as A  # noqa: E402

VS = (40, 4, 4)


def test_reference_trilinear_matches_scipy():
    from scipy.ndimage import map_coordinates
    rng = np.random.default_rng(0)
    crop = rng.integers(0, 256, (7, 19, 23), dtype=np.uint8)
    s = np.stack([rng.uniform(0, n - 1, (4, 9, 11)) for n in crop.shape]).astype(np.float32)
    want = map_coordinates(crop.astype(np.float64), s.astype(np.float64), order=1)
    assert np.abs(R.trilinear_f64(s, crop) - want).max() < 1e-10
    assert np.abs(R.sample_raw(s, crop) - (want * 2 / 255 - 1)).max() < 1e-12


def test_reference_nearest_matches_scipy_away_from_ties():
    from scipy.ndimage import map_coordinates
    rng = np.random.default_rng(1)
    crop = rng.integers(1, 2 ** 40, (7, 19, 23), dtype=np.int64)
    s = np.stack([rng.uniform(0, n - 1, (4, 9, 11)) for n in crop.shape]).astype(np.float32)
    frac = s - np.floor(s)
    away = (np.abs(frac - 0.5) > 1e-3).all(axis=0)
    assert away.mean() > 0.9
    # scipy interpolates in float64, so the ids go through an index volume instead
    index = np.arange(crop.size, dtype=np.float64).reshape(crop.shape)
    want = crop.ravel()[map_coordinates(index, s.astype(np.float64), order=0).astype(np.int64)]
    assert np.array_equal(R.sample_nearest(s, crop)[away], want[away])


def test_nearest_rule_is_float32_floor_of_s_plus_half():
    crop = np.arange(2 * 3 * 8, dtype=np.int64).reshape(2, 3, 8)
    s = np.zeros((3, 1, 1, 4), dtype=np.float32)
    s[2, 0, 0] = [2.5, np.nextafter(np.float32(2.5), np.float32(0)), 3.4999998, -3.0]   # tie goes up; one ulp below stays; clamp
    assert R.sample_nearest(s, crop)[0, 0].tolist() == [3, 2, 3, 0]


def test_source_box_contains_the_map_for_50_drawn_plans():
    rng = np.random.default_rng(5)
    params = A.AugParams(deform_p=1.0, shift_p=1.0)
    for k in range(50):
        shape = (int(rng.integers(1, 9)),) + (int(rng.integers(8, 40)),) * 2
        plan = A.draw_plan(rng, params, shape, VS)
        lo, hi = A.source_box(plan)
        assert R.box_contains(lo, hi, R.map_f64(plan, lo)), (k, shape)
        # a region: the centre of the block; its box is no larger and contains the map there
        off = tuple(n // 4 for n in shape)
        sub = tuple(max(1, n - 2 * o) for n, o in zip(shape, off))
        rlo, rhi = A.source_box(plan, (off, sub))
        s = R.map_f64(plan, rlo)[(slice(None),) + tuple(slice(o, o + n) for o, n in zip(off, sub))]
        assert R.box_contains(rlo, rhi, s)
        assert all(a >= b for a, b in zip(rlo, lo)) and all(a <= b for a, b in zip(rhi, hi))


def test_identity_plan_box_is_the_block_plus_margin():
    lo, hi = A.source_box(A.AugPlan((5, 24, 24)))
    assert lo == (-1, -1, -1) and hi == (7, 26, 26)


def test_draw_plan_is_deterministic_and_draws_nothing_when_off():
    a = A.draw_plan(np.random.default_rng(9), A.AugParams(deform_p=1.0, shift_p=1.0), (6, 20, 20), VS)
    b = A.draw_plan(np.random.default_rng(9), A.AugParams(deform_p=1.0, shift_p=1.0), (6, 20, 20), VS)
    assert a.mirror == b.mirror and a.swap == b.swap and a.u == b.u and a.theta == b.theta
    assert np.array_equal(a.lattice, b.lattice) and np.array_equal(a.shifts, b.shifts) and np.array_equal(a.linear, b.linear)
    assert a.lattice.dtype == np.float32 and a.shifts.dtype == np.int32 and a.shifts.shape == (2, 6)
    # reference arguments at voxel size (40, 4, 4): nodes every (4, 40, 40) voxels, one beyond the block on each side
    assert a.lattice.shape == (3,) + A.lattice_shape((6, 20, 20), (4.0, 40.0, 40.0)) == (3, 5, 4, 4)
    assert np.allclose(a.inv_spacing, [1 / 4, 1 / 40, 1 / 40]) and 0.9 <= a.u <= 1.1 and 0 <= a.theta < 2 * np.pi
    c = A.draw_plan(np.random.default_rng(10), A.AugParams(deform_p=1.0, shift_p=1.0), (6, 20, 20), VS)
    assert not np.array_equal(a.lattice, c.lattice)
    rng = np.random.default_rng(3)
    before = rng.bit_generator.state
    off = A.draw_plan(rng, A.AugParams(simple=False, deform_p=0.0, shift_p=0.0), (6, 20, 20), VS)
    assert rng.bit_generator.state == before
    assert off.mirror == (False, False, False) and not off.swap and off.lattice is None and off.shifts is None
    assert off.linear.tolist() == [1, 1, 0, 0, 1]


def test_shift_rule_steps_accumulate_and_slips_do_not():
    rng = np.random.default_rng(2)
    p = A.draw_plan(rng, A.AugParams(simple=False, deform_p=0.0, shift_p=1.0, prob_shift=1.0, prob_slip=0.0), (50, 8, 8), VS)
    steps = np.diff(np.concatenate([np.zeros((2, 1), dtype=np.int32), p.shifts], axis=1), axis=1)
    assert 2.0 < steps.std() < 4.0 and np.abs(p.shifts[:, -1]).max() > 3          # a random walk of sigma-3 steps
    p = A.draw_plan(rng, A.AugParams(simple=False, deform_p=0.0, shift_p=1.0, prob_shift=0.0, prob_slip=0.2), (400, 8, 8), VS)
    moved = (p.shifts != 0).any(axis=0).mean()
    assert 0.1 < moved < 0.3                                                      # slips stay in their own section


def test_refusals_of_the_plan():
    with pytest.raises(ValueError, match="square"):
        A.draw_plan(np.random.default_rng(0), A.AugParams(), (4, 16, 20), VS)
    with pytest.raises(NotImplementedError, match="voxel_size"):
        A.draw_plan(np.random.default_rng(0), A.AugParams(simple=False, deform_p=1.0), (4, 16, 16), (40, 4, 8))
    A.draw_plan(np.random.default_rng(0), A.AugParams(simple=False, deform_p=1.0, rotate=False), (4, 16, 20), (40, 4, 8))
    with pytest.raises(ValueError, match="at most 4096"):
        A.draw_plan(np.random.default_rng(0), A.AugParams(deform_p=1.0, control_point_spacing=(40, 4, 4)), (30, 64, 64), VS)


def test_toml_key_parsing():
    assert A.AugParams.from_config(None) is None and A.AugParams.from_config(False) is None
    d = A.AugParams.from_config(True)
    assert (d.simple, d.deform_p, d.scale_interval, d.rotate, d.shift_p, d.prob_slip, d.prob_shift, d.shift_sigma) == \
        (True, 0.5, (0.9, 1.1), True, 0.5, 0.2, 0.2, 3.0)
    assert d.control_point_spacing is None and d.jitter_sigma is None
    p = A.AugParams.from_config({"deform_p": 1, "scale_interval": [0.8, 1.2], "rotate": False, "control_point_spacing": [80, 80, 80],
                                 "jitter_sigma": [0, 8, 8], "shift_p": 0.25, "prob_slip": 0.1, "prob_shift": 0.3, "shift_sigma": 2, "simple": False})
    assert p == A.AugParams(False, 1.0, (0.8, 1.2), False, (80.0, 80.0, 80.0), (0.0, 8.0, 8.0), 0.25, 0.1, 0.3, 2.0)
    with pytest.raises(ValueError, match="unknown augment key.*subsample"):
        A.AugParams.from_config({"subsample": 4})
    with pytest.raises(ValueError, match="probability"):
        A.AugParams.from_config({"deform_p": 1.5})
    with pytest.raises(ValueError, match="augment must be"):
        A.AugParams.from_config("yes")


def test_make_sample_source_refuses_what_is_not_built(tmp_path):
    from bootstrapper_amd.train import make_sample_source
    two_d = {"input_shape": [64, 64], "output_shape": [32, 32], "downsample_factors": [[2, 2]],
             "outputs": {"2d_affs": {"dims": 2, "neighborhood": [[-1, 0], [0, -1]]}}}
    with pytest.raises(NotImplementedError, match="2-D setups"):
        make_sample_source({"samples": [], "augment": True}, two_d)
    second = {"input_shape": [8, 32, 32], "output_shape": [4, 16, 16], "inputs": {"3d_lsds": {"sigma": 8}},
              "outputs": {"3d_affs": {"dims": 3, "neighborhood": [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]}}}
    with pytest.raises(NotImplementedError, match="synthetic labels"):
        make_sample_source({"synthetic_labels": True, "augment": {"deform_p": 0.3}}, second)
    first = {"input_shape": [8, 32, 32], "output_shape": [4, 16, 16],
             "outputs": {"3d_affs": {"dims": 3, "neighborhood": [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]}}}
    with pytest.raises(ValueError, match="unknown augment key.*jitter"):
        make_sample_source({"samples": [], "augment": {"jitter": 2}}, first)


@pytest.fixture(scope="module")
def emulated_case():
    """block (5, 24, 24), lattice spacing 4 with shifts beyond it: the case in which each of the faults shows"""
    plan = R.build_plan(R.BLOCKS["5x24x24"], 4.0, seed=11)
    lo, hi = A.source_box(plan)
    raw, labels, mask = R.build_crops(tuple(h - l for l, h in zip(lo, hi)), seed=12)
    return plan, lo, labels


@pytest.mark.parametrize("block", sorted(R.BLOCKS))
@pytest.mark.parametrize("spacing", sorted(R.SPACINGS))
def test_emulated_kernel_passes_the_derived_gate(block, spacing):
    """float32 numpy, no fused multiply-add: the gate of the GPU test holds for the arithmetic it was derived for"""
    plan = R.build_plan(R.BLOCKS[block], R.SPACINGS[spacing], seed=11)
    lo, _ = A.source_box(plan)
    excess, worst = R.coords_excess(R.emulate_coords(plan, lo), plan, lo)
    assert excess <= 1.0, (excess, worst)
    if spacing == "spacing4":   # the case is what it claims: r leaves the lattice on both sides
        r_y = np.arange(plan.shape[1])[None, :] + plan.shifts[0][:, None]
        r_x = np.arange(plan.shape[2])[None, :] + plan.shifts[1][:, None]
        n = plan.lattice.shape[1:]
        assert (r_x.min() + 4) < 0 and r_y.max() / 4.0 + 1 > n[1] - 1
    else:
        assert plan.lattice.shape[2:] == (4, 4)


@pytest.mark.parametrize("fault", R.FAULTS[:4])
def test_injected_coordinate_faults_are_caught(emulated_case, fault):
    plan, lo, _ = emulated_case
    excess, _ = R.coords_excess(R.emulate_coords(plan, lo, fault), plan, lo)
    assert excess > 1.0, fault


def test_injected_label_fault_is_caught(emulated_case):
    """labels are compared bit for bit with the reference sampling the same coordinates over the same region"""
    plan, lo, labels = emulated_case
    coords = R.emulate_coords(plan, lo)
    ctx, out = (1, 4, 4), (3, 16, 16)
    want = R.sample_nearest(coords, labels, (ctx, out))
    assert np.array_equal(R.emulate_labels(coords, labels, ctx, out), want)
    assert not np.array_equal(R.emulate_labels(coords, labels, ctx, out, "ctx_dropped"), want)


def test_exact_cases_of_the_reference():
    """identity, mirror, swap and integer shifts are numpy slices, flips and transposes of the crop (the same statements
    tests/test_aug_gpu.py makes about the device)"""
    shape = (5, 24, 24)
    lo = (-2, -8, -8)
    _, labels, _ = R.build_crops((9, 40, 40), seed=3)
    centre = labels[2:7, 8:32, 8:32]
    ident = R.sample_nearest(R.map_f64(A.AugPlan(shape), lo).astype(np.float32), labels)
    assert np.array_equal(ident, centre)
    mir = R.sample_nearest(R.map_f64(A.AugPlan(shape, mirror=(True, False, True)), lo).astype(np.float32), labels)
    assert np.array_equal(mir, centre[::-1, :, ::-1])
    swp = R.sample_nearest(R.map_f64(A.AugPlan(shape, swap=True), lo).astype(np.float32), labels)
    assert np.array_equal(swp, centre.transpose(0, 2, 1))


def test_alignment_condition_is_met_by_the_reference_alone():
    """tests/test_train_aug_gpu.py checks raw against the label's value wherever the 3 x 3 x 3 neighbourhood of the augmented
    labels is uniform, and requires that share to be at least 20 % of the block.  Its store, boxes of side (12, 32, 32) in a
    volume of (36, 192, 192), meets that for the batches it draws (same seed, same draw order: sample, location, plan) through
    aug_ref alone, with a margin for the voxels the device may round to the other side, and there raw is the label's value."""
    import test_train_aug_gpu as T
    raw, labels = R.boxes_volume(T.VOLUME, T.BOX)
    assert min(T.BOX) >= 8 and labels.max() > 20
    rng = np.random.default_rng(42)
    ctx = [(i - o) // 2 for i, o in zip(T.INPUT, T.OUTPUT)]
    shares = []
    params = A.AugParams.from_config(T.ALIGN)
    for _ in range(T.BATCHES):
        rng.integers(1)
        off = [int(rng.integers(0, s - o + 1)) for s, o in zip(T.VOLUME, T.OUTPUT)]
        plan = A.draw_plan(rng, params, T.INPUT, T.VOXEL_SIZE)
        lo, hi = A.source_box(plan)
        start = [a - c + l for a, c, l in zip(off, ctx, lo)]
        size = [h - l for l, h in zip(lo, hi)]
        crops = []
        for vol in (raw, labels.astype(np.int64)):
            crop = np.zeros(size, dtype=vol.dtype)
            src = tuple(slice(max(a, 0), min(a + n, m)) for a, n, m in zip(start, size, vol.shape))
            dst = tuple(slice(s.start - a, s.stop - a) for s, a in zip(src, start))
            crop[dst] = vol[src]
            crops.append(crop)
        coords = R.map_f64(plan, lo).astype(np.float32)
        region = (ctx, T.OUTPUT)
        share, err = R.alignment(R.sample_raw(coords, crops[0], region), R.sample_nearest(coords, crops[1], region))
        assert err <= R.RAW_GATE
        shares.append(share)
    assert min(shares) >= 0.25, shares
