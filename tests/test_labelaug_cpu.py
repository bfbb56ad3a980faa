"""The geometric augmentation of the synthetic labels without a GPU and without a library call: the train config key
`label_augment` and its defaults (bootstrapper_amd/augment_labels.py), the refusals by name, the construction of the source and
its random streams, and the rule "labels are 0 outside the block" on the float32 emulation of the coordinate launch
(tests/aug_ref.py): the padded nearest sampling the device runs against the rule written without padding (tests/labelaug_ref.py),
which a sampler that clamps to the block must not pass."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_ref as R  # noqa: E402
import labelaug_ref as L  # noqa: E402
from bootstrapper_amd import augment as A  # noqa: E402
from bootstrapper_amd import augment_labels as AL  # noqa: E402

SECOND = {"input_shape": [21, 100, 100], "output_shape": [1, 8, 8],
          "outputs": {"3d_affs": {"dims": 3, "neighborhood": [[-1, 0, 0], [0, -1, 0], [0, 0, -1]], "grow_boundary": 1}},
          "inputs": {"2d_lsds": {"dims": 6, "sigma": 10, "downsample": 2, "grow_boundary": 1},
                     "2d_affs": {"dims": 6, "neighborhood": [[-1, 0], [0, -1], [-9, 0], [0, -9], [-27, 0], [0, -27]], "grow_boundary": 1}}}
FIRST = {"input_shape": [8, 32, 32], "output_shape": [4, 16, 16], "outputs": {"3d_affs": {"dims": 3, "neighborhood": [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]}}}
TWO_D = {"input_shape": [32, 32], "output_shape": [16, 16], "downsample_factors": [[2, 2]], "outputs": {"2d_affs": {"dims": 2}}}
SYNTH = {"synthetic_labels": True, "voxel_size": [40, 4, 4]}


def test_defaults_are_the_second_stage_call_sites():
    assert AL.LabelAugParams.from_config(None) is None and AL.LabelAugParams.from_config(False) is None
    d = AL.LabelAugParams.from_config(True)
    assert d == AL.LabelAugParams()
    assert (d.simple, d.deform_p, d.scale_interval, d.rotate, d.control_point_spacing, d.jitter_sigma, d.shift_p, d.prob_slip, d.prob_shift,
            d.shift_sigma) == (True, 1.0, (0.8, 1.2), True, None, None, 0.8, 0.1, 0.1, 3.0)
    assert "intensity" not in [f.name for f in __import__("dataclasses").fields(AL.LabelAugParams)]
    for vs in ((40, 4, 4), (8, 8, 8)):
        p = d.to_aug_params(vs)
        assert isinstance(p, A.AugParams) and p.intensity is None
        assert [c / v for c, v in zip(p.control_point_spacing, vs)] == [4.0, 10.0, 10.0]
        assert [s / v for s, v in zip(p.jitter_sigma, vs)] == [1.0, 2.0, 2.0]
        assert (p.simple, p.deform_p, p.scale_interval, p.rotate, p.shift_p, p.prob_slip, p.prob_shift, p.shift_sigma) == \
            (True, 1.0, (0.8, 1.2), True, 0.8, 0.1, 0.1, 3.0)


def test_overrides_round_trip():
    table = {"simple": False, "deform_p": 0.25, "scale_interval": [0.9, 1.1], "rotate": False, "control_point_spacing": [80, 20, 24],
             "jitter_sigma": [0, 4, 4], "shift_p": 0.5, "prob_slip": 0.2, "prob_shift": 0.3, "shift_sigma": 2}
    p = AL.LabelAugParams.from_config(table)
    assert p == AL.LabelAugParams(False, 0.25, (0.9, 1.1), False, (80.0, 20.0, 24.0), (0.0, 4.0, 4.0), 0.5, 0.2, 0.3, 2.0)
    q = p.to_aug_params((40, 4, 4))
    assert q == A.AugParams(False, 0.25, (0.9, 1.1), False, (80.0, 20.0, 24.0), (0.0, 4.0, 4.0), 0.5, 0.2, 0.3, 2.0, None)


def test_config_refusals_by_name():
    with pytest.raises(ValueError, match=r"unknown label_augment key\(s\) intensity"):
        AL.LabelAugParams.from_config({"intensity": True})
    with pytest.raises(ValueError, match=r"unknown label_augment key\(s\) noise_p, sigma; known: simple"):
        AL.LabelAugParams.from_config({"sigma": 2, "noise_p": 0.1})
    with pytest.raises(ValueError, match="label_augment must be true, false or a table"):
        AL.LabelAugParams.from_config(3)
    with pytest.raises(ValueError, match=r"label_augment\.deform_p.*a number"):
        AL.LabelAugParams.from_config({"deform_p": "often"})
    with pytest.raises(ValueError, match=r"label_augment\.scale_interval.*two"):
        AL.LabelAugParams.from_config({"scale_interval": 1.1})
    with pytest.raises(ValueError, match=r"label_augment\.simple.*true or false"):
        AL.LabelAugParams.from_config({"simple": 1})
    with pytest.raises(ValueError, match=r"label_augment\.shift_p.*a probability"):
        AL.LabelAugParams.from_config({"shift_p": 2})
    with pytest.raises(ValueError, match=r"label_augment\.scale_interval.*low <= high"):
        AL.LabelAugParams.from_config({"scale_interval": [1.2, 0.8]})
    with pytest.raises(ValueError, match=r"label_augment\.control_point_spacing.*three"):
        AL.LabelAugParams.from_config({"control_point_spacing": [40, 0, 4]})
    with pytest.raises(ValueError, match=r"other\.rotate"):
        AL.LabelAugParams.from_config({"rotate": "yes"}, key="other")


def test_block_refusals_by_name():
    from bootstrapper_amd.train import SyntheticSource
    d = AL.LabelAugParams()
    assert AL.check_block(d, (24, 148, 148), (40, 4, 4)) == (9, 18, 18)          # the shipped block: 2916 nodes
    assert AL.check_block(d, (21, 100, 100), (40, 4, 4)) == (8, 13, 13) and AL.check_block(d, (22, 100, 100), (8, 8, 8)) == (9, 13, 13)
    assert 9 * 18 * 18 <= A.MAX_LATTICE_NODES
    oblong = dict(SECOND, input_shape=[21, 100, 96])
    with pytest.raises(ValueError, match=r"square.*set label_augment\.simple = false"):
        SyntheticSource(oblong, (40, 4, 4), label_augment=True)
    assert SyntheticSource(oblong, (40, 4, 4), label_augment=AL.LabelAugParams(simple=False)).label_augment.simple is False
    with pytest.raises(NotImplementedError, match=r"voxel_size\[1\] == voxel_size\[2\].*set label_augment\.rotate = false"):
        SyntheticSource(SECOND, (40, 4, 8), label_augment=True)
    assert SyntheticSource(SECOND, (40, 4, 8), label_augment=AL.LabelAugParams(rotate=False)).label_rng is not None
    with pytest.raises(ValueError, match=r"at most 4096.*label_augment\.control_point_spacing"):
        SyntheticSource(SECOND, (40, 4, 4), label_augment=AL.LabelAugParams(control_point_spacing=(40.0, 4.0, 4.0)))   # 1 voxel
    # without DeformAugment neither the voxel size nor the lattice matters
    off = AL.LabelAugParams(deform_p=0.0, control_point_spacing=(40.0, 4.0, 4.0))
    assert AL.check_block(off, (21, 100, 100), (40, 4, 8)) is None


def test_key_goes_with_synthetic_labels_only():
    from bootstrapper_amd.train import make_sample_source
    with pytest.raises(NotImplementedError, match=r"label_augment.*3d_affs_from_2d_mtlsd.*synthetic_labels = true"):
        make_sample_source({"label_augment": True}, SECOND)
    with pytest.raises(NotImplementedError, match=r"label_augment: not built for the 3d_affs setup.*`augment` and `augment2d`"):
        make_sample_source({"samples": [], "label_augment": True}, FIRST)
    with pytest.raises(NotImplementedError, match=r"label_augment: not built for the 2d_affs setup.*`augment` and `augment2d`"):
        make_sample_source({"samples": [], "label_augment": True}, TWO_D)
    with pytest.raises(ValueError, match="unknown label_augment key.*sigma"):
        make_sample_source(dict(SYNTH, label_augment={"sigma": 2}), SECOND)
    # `augment` and `augment2d` on these setups stay refused with exactly today's messages
    with pytest.raises(NotImplementedError, match="augment: not built for synthetic labels"):
        make_sample_source(dict(SYNTH, augment=True, label_augment=True), SECOND)
    with pytest.raises(NotImplementedError, match="augment2d: not built"):
        make_sample_source(dict(SYNTH, augment2d=True, label_augment=True), SECOND)


def plan_of(src):
    return A.draw_plan(src.label_rng, src.label_params, src.inp, src.vs)


def same_plan(a, b):
    return (a.mirror == b.mirror and a.swap == b.swap and a.u == b.u and a.theta == b.theta and np.array_equal(a.lattice, b.lattice)
            and (a.shifts is None) == (b.shifts is None) and (a.shifts is None or np.array_equal(a.shifts, b.shifts)))


def test_construction_and_streams():
    """the constructor of the source touches no GPU; the plans come from (seed, 2), the other two streams are not touched"""
    import random
    from bootstrapper_amd.train import SyntheticSource, make_sample_source
    table = {"scale_interval": [0.9, 1.1], "shift_p": 1}
    a, b, other = (make_sample_source(dict(SYNTH, label_augment=table), SECOND, rank=r) for r in (0, 0, 1))
    assert isinstance(a, SyntheticSource) and a.label_augment == AL.LabelAugParams(scale_interval=(0.9, 1.1), shift_p=1.0)
    assert a.label_params == a.label_augment.to_aug_params((40.0, 4.0, 4.0)) and a.input_augment is None and a.aug_rng is None and a.engine is None
    mine = np.random.default_rng((42, 2))
    for _ in range(3):
        pa, pb, po = plan_of(a), plan_of(b), plan_of(other)
        want = A.draw_plan(mine, a.label_params, (21, 100, 100), (40.0, 4.0, 4.0))
        assert same_plan(pa, pb) and same_plan(pa, want) and not same_plan(pa, po)
        assert pa.lattice.shape == (3, 8, 13, 13) and pa.shifts.shape == (2, 21) and 0.9 <= pa.u <= 1.1
    assert plan_of(make_sample_source(dict(SYNTH, label_augment=True), SECOND, rank=1)).lattice.shape == (3, 8, 13, 13)
    plain = make_sample_source(SYNTH, SECOND)
    assert plain.label_augment is None and plain.label_rng is None and plain.label_params is None
    assert make_sample_source(dict(SYNTH, label_augment=False), SECOND).label_augment is None
    assert SyntheticSource(SECOND, (40, 4, 4), label_augment=True).label_augment == AL.LabelAugParams()
    # random.Random(seed) delivers the same next value with and without the key, and so does (seed, 1) beside it
    both = make_sample_source(dict(SYNTH, label_augment=True, input_augment=True), SECOND)
    only_in = make_sample_source(dict(SYNTH, input_augment=True), SECOND)
    assert plain.rng.random() == make_sample_source(dict(SYNTH, label_augment=True), SECOND).rng.random() == both.rng.random() == random.Random(42).random()
    assert both.aug_rng.random() == only_in.aug_rng.random() == np.random.default_rng((42, 1)).random()
    assert both.label_rng.random() == np.random.default_rng((42, 2)).random()


def noise_labels(shape, seed=5):
    return R.build_crops(shape, seed)[1]


@pytest.mark.parametrize("block", sorted(R.BLOCKS))
@pytest.mark.parametrize("spacing", sorted(R.SPACINGS))
def test_padded_sampling_is_the_rule(block, spacing):
    shape = R.BLOCKS[block]
    plan = R.build_plan(shape, R.SPACINGS[spacing], seed=11)
    lab = noise_labels(shape)
    coords = R.emulate_coords(plan, L.BOX_LO)
    want = L.rule(coords, lab)
    share = float((want == 0).mean())
    print(f"{block} {spacing}: {100 * share:.1f} % of the voxels lie outside the block")
    assert 0.0 < share < 1.0                                   # both branches of the rule
    assert np.array_equal(L.padded(coords, lab), want)
    assert set(np.unique(want)) <= set(np.unique(lab)) | {0}
    assert not np.array_equal(L.clamping(coords, lab), want)   # a sampler that clamps to the block smears the border: refused
    assert (L.clamping(coords, lab) != 0).all()


@pytest.mark.parametrize("block", sorted(R.BLOCKS))
def test_mild_plan_lets_a_frame_of_zeros_in(block):
    shape = R.BLOCKS[block]
    lab = noise_labels(shape)
    coords = R.emulate_coords(L.mild_plan(shape), L.BOX_LO)
    want = L.rule(coords, lab)
    assert np.array_equal(L.padded(coords, lab), want) and not np.array_equal(L.clamping(coords, lab), want)
    zero = want == 0
    # the map is separable, so the zeros are a frame: per axis the voxels whose source index leaves the block
    per = [zero.all(axis=tuple(b for b in range(3) if b != a)) for a in range(3)]
    assert np.array_equal(zero, per[0][:, None, None] | per[1][None, :, None] | per[2][None, None, :])
    for a, n in enumerate(shape):
        c = (n - 1) / 2.0
        far = np.abs(np.arange(n) - c) * 1.2 > c + 0.75         # clearly outside: more than a quarter voxel beyond the last centre's cell
        near = np.abs(np.arange(n) - c) * 1.2 < c + 0.25
        assert per[a][far].all() and not per[a][near].any(), a
    assert 0.0 < zero.mean() < 1.0


def test_identity_and_integer_shift_plans():
    shape = (5, 24, 24)
    lab = noise_labels(shape)
    ident = A.AugPlan(shape)
    assert AL.is_identity(ident) and AL.is_identity(A.AugPlan(shape, u=1.0, theta=0.0))
    assert np.array_equal(L.padded(R.emulate_coords(ident, L.BOX_LO), lab), lab) and np.array_equal(L.rule(R.emulate_coords(ident, L.BOX_LO), lab), lab)
    shifts = np.array([[0, 3, -8, 8, 1], [-7, 0, 8, -2, -30]], dtype=np.int32)
    plan = A.AugPlan(shape, shifts=shifts)
    coords = R.emulate_coords(plan, L.BOX_LO)
    want = L.shifted_expected(lab, shifts)
    assert np.array_equal(L.rule(coords, lab), want) and np.array_equal(L.padded(coords, lab), want)
    assert (want[4] == 0).all() and (want[2, :8] == 0).all() and (want[2, :, -8:] == 0).all() and (want[0, :, :7] == 0).all()    # zeros enter, not replicated edges
    assert not np.array_equal(L.clamping(coords, lab), want)
    for other in (A.AugPlan(shape, mirror=(False, True, False)), A.AugPlan(shape, swap=True), plan, A.AugPlan(shape, u=1.2),
                  A.AugPlan(shape, theta=0.3), A.AugPlan(shape, lattice=np.zeros((3, 1, 1, 1), np.float32), inv_spacing=np.ones(3, np.float32))):
        assert not AL.is_identity(other)


def test_nan_and_far_coordinates_give_zero():
    lab = noise_labels((3, 4, 5))
    coords = np.zeros((3, 3, 4, 5), dtype=np.float32) + 2.0
    coords[0, 0] = np.nan
    coords[1, 1] = 1e30
    coords[2, 2] = -1e30
    out = L.rule(coords, lab)
    assert (out[:, :, :] == 0).all()
    coords[:] = 2.0
    assert (L.rule(coords, lab) == lab[1, 1, 1]).all()


def test_warp_labels_refuses_before_any_launch():
    torch = pytest.importorskip("torch")
    plan = A.AugPlan((2, 4, 4))
    with pytest.raises(ValueError, match="int64 CUDA"):
        AL.warp_labels(torch.zeros((2, 4, 4), dtype=torch.int64), plan)                 # not on the device
    with pytest.raises(ValueError, match="int64 CUDA"):
        AL.warp_labels(np.zeros((2, 4, 4), dtype=np.int64), plan)


def test_constants():
    from bootstrapper_amd.train import SyntheticSource as S
    assert "DeformAugment" in S.NOT_BUILT and "DeformAugment" in S.NOT_BUILT_WITH_INPUT_AUGMENT
    assert "DeformAugment" not in S.NOT_BUILT_WITH_LABEL_AUGMENT and "DeformAugment" not in S.NOT_BUILT_WITH_BOTH
    assert "SimpleAugment" not in S.NOT_BUILT_WITH_LABEL_AUGMENT + S.NOT_BUILT_WITH_BOTH and "ShiftAugment" not in S.NOT_BUILT_WITH_LABEL_AUGMENT + S.NOT_BUILT_WITH_BOTH
    assert "NoiseAugment" in S.NOT_BUILT_WITH_LABEL_AUGMENT and "NoiseAugment" not in S.NOT_BUILT_WITH_BOTH and "artifact" in S.NOT_BUILT_WITH_BOTH
    assert "synthetic labels" not in A.NOT_BUILT_WITH_INTENSITY.split("(")[0] and "label_augment" in A.NOT_BUILT_WITH_INTENSITY
