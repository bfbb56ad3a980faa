"""The input augmentation of the second-stage setups without a GPU: the host's draws (bootstrapper_amd/augment_inputs.py), the
train config key and its refusals, the per-section taps, the channel blur of the reference's smoothing call, and the
comparisons of tests/test_augin_gpu.py run on a float32 emulation of the launches -- which they must pass, and must not pass
with any of the injected faults."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augin_ref as R  # noqa: E402
from bootstrapper_amd import augment_inputs as A  # noqa: E402


class Recorder:
    """a numpy Generator that notes every draw"""

    def __init__(self, seed):
        self.rng, self.calls = np.random.default_rng(seed), []

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name,) + tuple(x for x in a if isinstance(x, (int, tuple))))
            return getattr(self.rng, name)(*a, **k)
        return call


ALWAYS = dict(noise_p=1.0, channel_intensity_p=1.0, section_intensity_p=1.0, smooth_p=1.0, prob_low_contrast=0.5)
OFF = dict(noise_p=0.0, channel_intensity_p=0.0, section_intensity_p=0.0, smooth_p=0.0, prob_low_contrast=0.0)


def test_draw_order():
    c, d = 6, 5
    rec = Recorder(3)
    plan = A.draw_input_plan(rec, A.InputAugParams(**ALWAYS), (c, d, 8, 8))
    # noise coin; channel coin + C scales + C shifts; section coin + D scales + D shifts; smooth coin + D sigmas; D values r; seed
    assert rec.calls == [("random",), ("random",), ("uniform", c), ("uniform", c), ("random",), ("uniform", d), ("uniform", d),
                         ("random",), ("uniform", d), ("random", d), ("integers", 0, 2 ** 64)], rec.calls
    assert plan.applied and plan.noise_sigma == float(np.float32(0.1)) and 0 < plan.seed < 2 ** 64
    assert plan.channel_scale.shape == plan.channel_shift.shape == (c,) and plan.section_scale.shape == plan.section_shift.shape == (d,)
    assert plan.channel_scale.dtype == plan.section_shift.dtype == np.float32
    assert 0.9 <= min(plan.channel_scale.min(), plan.section_scale.min()) and max(plan.channel_scale.max(), plan.section_scale.max()) <= 1.1
    assert max(np.abs(plan.channel_shift).max(), np.abs(plan.section_shift).max()) <= 0.1
    assert plan.sigma.shape == (d,) and 0.1 <= plan.sigma.min() and plan.sigma.max() <= 1.5
    assert plan.weights.shape == (d, 13) and plan.weights.dtype == np.float32 and plan.radius.dtype == np.int32
    assert plan.radius.tolist() == [int(4 * s + 0.5) for s in plan.sigma]
    assert plan.low_contrast is None or (plan.low_contrast.dtype == np.int32 and set(plan.low_contrast.tolist()) <= {0, 3})


def test_a_node_that_is_off_takes_no_draw():
    rec = Recorder(3)
    plan = A.draw_input_plan(rec, A.InputAugParams(**OFF), (3, 4, 8, 8))
    assert rec.calls == [] and not plan.applied
    for key, draws in (("noise_p", ["random", "integers"]), ("channel_intensity_p", ["random", "uniform", "uniform"]),
                       ("section_intensity_p", ["random", "uniform", "uniform"]), ("smooth_p", ["random", "uniform"])):
        rec = Recorder(3)
        A.draw_input_plan(rec, A.InputAugParams(**dict(OFF, **{key: 1.0})), (3, 4, 8, 8))
        assert [c[0] for c in rec.calls] == draws, key
    rec = Recorder(3)
    plan = A.draw_input_plan(rec, A.InputAugParams(**dict(OFF, prob_low_contrast=1.0)), (3, 4, 8, 8))
    assert rec.calls == [("random", 4)] and plan.low_contrast.tolist() == [3, 3, 3, 3] and plan.applied
    # a coin that falls the other way draws nothing more; a smoothing of radius 0 everywhere changes nothing
    rec = Recorder(3)
    plan = A.draw_input_plan(rec, A.InputAugParams(**dict(OFF, smooth_p=1.0, blur=(0.1, 0.12))), (3, 4, 8, 8))
    assert plan.radius.tolist() == [0] * 4 and not plan.applied
    # a seed for the same stream gives the same plan
    a = A.draw_input_plan(np.random.default_rng(9), A.InputAugParams(), (6, 4, 8, 8))
    b = A.draw_input_plan(np.random.default_rng(9), A.InputAugParams(), (6, 4, 8, 8))
    assert a.seed == b.seed and a.applied == b.applied and all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("channel_scale", "sigma", "low_contrast"))


def test_config_key():
    assert A.InputAugParams.from_config(None) is None and A.InputAugParams.from_config(False) is None
    d = A.InputAugParams.from_config(True)
    assert (d.noise_p, d.noise_var, d.channel_intensity_p, d.section_intensity_p, d.scale, d.shift, d.smooth_p, d.blur, d.smooth_channels,
            d.prob_low_contrast, d.contrast_scale) == (0.1, 0.01, 0.5, 0.5, (0.9, 1.1), (-0.1, 0.1), 0.5, (0.1, 1.5), True, 0.1, 0.1)
    p = A.InputAugParams.from_config({"noise_p": 1, "noise_var": 0.04, "scale": [0.8, 1.2], "blur": [1, 1.25], "smooth_channels": False})
    assert p == A.InputAugParams(noise_p=1.0, noise_var=0.04, scale=(0.8, 1.2), blur=(1.0, 1.25), smooth_channels=False)
    with pytest.raises(ValueError, match="unknown input_augment key.*gamma_p"):
        A.InputAugParams.from_config({"gamma_p": 0.5})
    with pytest.raises(ValueError, match="unknown input_augment key.*prob_missing"):
        A.InputAugParams.from_config({"prob_missing": 0.1})
    with pytest.raises(ValueError, match="probability"):
        A.InputAugParams.from_config({"smooth_p": 2})
    with pytest.raises(ValueError, match="blur"):
        A.InputAugParams.from_config({"blur": [0.5, 2.0]})
    with pytest.raises(ValueError, match="low <= high"):
        A.InputAugParams.from_config({"scale": [1.1, 0.9]})
    with pytest.raises(ValueError, match="true or false"):
        A.InputAugParams.from_config({"smooth_channels": 1})
    with pytest.raises(ValueError, match="true, false or a table"):
        A.InputAugParams.from_config(3)


SECOND = {"input_shape": [21, 100, 100], "output_shape": [1, 8, 8],
          "outputs": {"3d_affs": {"dims": 3, "neighborhood": [[-1, 0, 0], [0, -1, 0], [0, 0, -1]], "grow_boundary": 1}},
          "inputs": {"2d_lsds": {"dims": 6, "sigma": 10, "downsample": 2, "grow_boundary": 1},
                     "2d_affs": {"dims": 6, "neighborhood": [[-1, 0], [0, -1], [-9, 0], [0, -9], [-27, 0], [0, -27]], "grow_boundary": 1}}}
FIRST = {"input_shape": [8, 32, 32], "output_shape": [4, 16, 16], "outputs": {"3d_affs": {"dims": 3, "neighborhood": [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]}}}
TWO_D = {"input_shape": [32, 32], "output_shape": [16, 16], "downsample_factors": [[2, 2]], "outputs": {"2d_affs": {"dims": 2}}}


def test_config_reaches_the_source_and_refusals():
    """the constructor of the source touches no GPU"""
    from bootstrapper_amd.train import SyntheticSource, make_sample_source
    src = make_sample_source({"synthetic_labels": True, "voxel_size": [40, 4, 4], "input_augment": {"smooth_p": 1, "smooth_channels": False}}, SECOND, rank=1)
    assert isinstance(src, SyntheticSource) and src.input_augment == A.InputAugParams(smooth_p=1.0, smooth_channels=False)
    assert src.arrays == [("2d_lsds", 0, 6), ("2d_affs", 6, 12)]
    assert src.aug_rng.random() == np.random.default_rng((43, 1)).random()       # a stream of its own: (seed, 1)
    plain = make_sample_source({"synthetic_labels": True, "voxel_size": [40, 4, 4]}, SECOND)
    assert plain.input_augment is None and plain.aug_rng is None
    assert make_sample_source({"synthetic_labels": True, "input_augment": False}, SECOND).input_augment is None
    assert SyntheticSource(SECOND, (40, 4, 4), input_augment=True).input_augment == A.InputAugParams()
    with pytest.raises(ValueError, match="unknown input_augment key.*sigma"):
        make_sample_source({"synthetic_labels": True, "input_augment": {"sigma": 2}}, SECOND)
    with pytest.raises(NotImplementedError, match=r"input_augment.*3d_affs_from_2d_mtlsd.*synthetic_labels = true"):
        make_sample_source({"input_augment": True}, SECOND)                       # only together with synthetic labels
    with pytest.raises(NotImplementedError, match=r"input_augment: not built for the 3d_affs setup.*`augment`"):
        make_sample_source({"samples": [], "input_augment": True}, FIRST)
    with pytest.raises(NotImplementedError, match=r"input_augment: not built for the 2d_affs setup.*`augment2d`"):
        make_sample_source({"samples": [], "input_augment": True}, TWO_D)
    with pytest.raises(NotImplementedError, match="augment: not built for synthetic labels"):   # stays refused exactly as before
        make_sample_source({"synthetic_labels": True, "augment": True, "input_augment": True}, SECOND)
    with pytest.raises(NotImplementedError, match="augment2d: not built"):
        make_sample_source({"synthetic_labels": True, "augment2d": True, "input_augment": True}, SECOND)
    assert "DeformAugment" in SyntheticSource.NOT_BUILT and "NoiseAugment" in SyntheticSource.NOT_BUILT
    assert "DeformAugment" in SyntheticSource.NOT_BUILT_WITH_INPUT_AUGMENT and "NoiseAugment" not in SyntheticSource.NOT_BUILT_WITH_INPUT_AUGMENT


def test_section_taps_are_scipy_s():
    import scipy.ndimage
    sigma = np.array([0.1, 0.124, 0.5, 0.9, 1.5, 1.62])
    weights, radius = A.section_taps(sigma)
    assert weights.shape == (6, 13) and weights.dtype == np.float32 and radius.tolist() == [0, 0, 2, 4, 6, 6]
    for z, s in enumerate(sigma):
        r = int(radius[z])
        delta = np.zeros(4 * r + 1)
        delta[2 * r] = 1
        assert np.allclose(weights[z, :2 * r + 1], scipy.ndimage.gaussian_filter1d(delta, s)[r:3 * r + 1], rtol=1e-6, atol=0)
        assert (weights[z, 2 * r + 1:] == 0).all()
    assert weights[0, 0] == 1.0 and weights[1, 0] == 1.0
    with pytest.raises(ValueError, match="radius"):
        A.section_taps([1.7])


def test_the_reference_smoothing_blurs_across_channels():
    """gaussian_filter on the slab (C, 1, H, W) with a scalar sigma: the z pass is the identity, the c pass is not"""
    import scipy.ndimage
    x = np.random.default_rng(2).random((6, 1, 17, 33))
    for s in (0.5, 1.5):
        full = scipy.ndimage.gaussian_filter(x, s, mode="reflect")
        assert np.abs(full - scipy.ndimage.gaussian_filter(x, (s, 0, s, s), mode="reflect")).max() <= 1e-15
        assert np.abs(R.smooth(x.astype(np.float32), [s]) - scipy.ndimage.gaussian_filter(x.astype(np.float32).astype(np.float64), s, mode="reflect")).max() <= 1e-15
        plane = scipy.ndimage.gaussian_filter(x, (0, 0, s, s), mode="reflect")
        assert np.abs(full - plane).max() > 0.05
        assert np.abs(R.smooth(x.astype(np.float32), [s], channels=False) - plane).max() <= 1e-6
    assert np.array_equal(R.smooth(x.astype(np.float32), [0.1]), x.astype(np.float32).astype(np.float64))   # radius 0: the section as it is


def test_group_mean_gate_adds_one_eps_per_plane():
    shape = (6, 3, 24, 40)
    m = np.array([0.5])
    assert np.allclose(R.group_mean_gate(shape, 0, m) - R.mean_gate(shape[1:], m), 3 * R.EPS * 0.5 * R.SLACK)
    assert np.allclose(R.group_mean_gate(shape, 1, m) - R.mean_gate(shape[1:], m), 6 * R.EPS * 0.5 * R.SLACK)


@pytest.mark.parametrize("array,nodes", R.CASES)
def test_emulation_passes_the_comparisons(array, nodes):
    shape = R.ARRAYS[array]
    plan, x0, emu = R.build_plan(shape, nodes), R.build_array(shape), R.Emulation()
    R.check(R.staged(emu, x0, plan), plan, emu.chain(x0, plan), show=lambda s: None)


def test_cases_mix_the_radii_and_hold_the_special_planes():
    radii = set()
    for shape in R.ARRAYS.values():
        radii |= set(R.build_plan(shape, "smooth").radius.tolist())
        x = R.build_array(shape)
        assert (x[0, 0] == 0.5).all() and x.min() == 0.0 and x.max() == 1.0
        assert all(x[c].min() == 0.0 and x[c].max() == 1.0 for c in range(1, shape[0]))
        if shape[1] > 2:
            assert (x[:, 1] == 0).all()
    assert radii == {0, 2, 6}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_comparisons_catch_the_fault(fault):
    """each fault is caught, on every array it can show on, by the comparison of its own node"""
    node = {"axis_swapped": "channel:", "plane_mean": "channel_mean", "no_c_pass": "smooth", "one_sigma": "differs where the rule is exact|smooth",
            "mirror_c": "smooth", "contrast_plane_mean": "contrast:", "noise_per_channel": "noise", "stale_section_mean": "section_mean"}[fault]
    for name, shape in R.ARRAYS.items():
        if shape[1] == 1 and fault in ("one_sigma", "plane_mean"):
            continue   # one section: its taps are section 0's; a channel's only plane is the channel
        plan, x0, emu = R.build_plan(shape, "all"), R.build_array(shape), R.Emulation(fault)
        with pytest.raises(AssertionError, match=node):
            R.check(R.staged(emu, x0, plan), plan, emu.chain(x0, plan), show=lambda s: None)
