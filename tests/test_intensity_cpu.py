"""The intensity augmentation without a GPU: the random numbers of tests/intensity_ref.py against a known answer and their
distributions, the host's draws (bootstrapper_amd/augment.py), the train config key, and the comparisons of
tests/test_intensity_gpu.py run on a float32 emulation of the launches -- which they must pass, and must not pass with
any of the injected faults."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import intensity_ref as R  # noqa: E402
from bootstrapper_amd import augment as A  # noqa: E402

N = 2 ** 16
SEED = 0x0123456789ABCDEF


def test_philox_known_answer():
    """Random123's kat_vectors, philox4x32 with 10 rounds: counter 0, key 0; and the all-ones vector of the same file"""
    assert tuple(int(v) for v in R.philox([0], 0)[:, 0]) == R.KNOWN_ANSWER
    # two counters at once give what each gives alone, and the key's halves are not interchangeable
    both = R.philox([0, 1], SEED)
    assert np.array_equal(both[:, 1], R.philox([1], SEED)[:, 0]) and not np.array_equal(both[:, 0], both[:, 1])
    assert not np.array_equal(R.philox([0], SEED), R.philox([0], (SEED >> 32) | ((SEED & 0xFFFFFFFF) << 32)))


@pytest.fixture(scope="module")
def words():
    return R.philox(np.arange(N), SEED)


def test_normals_have_zero_mean_and_unit_variance(words):
    n = R.normals(words)
    assert np.isfinite(n).all()
    mean, var = float(n.mean()), float(n.var())
    print(f"mean {mean:+.5f} (standard error {1 / np.sqrt(N):.5f}), variance {var:.5f} (standard error {np.sqrt(2 / N):.5f})")
    assert abs(mean) <= 5 / np.sqrt(N)
    assert abs(var - 1) <= 5 * np.sqrt(2 / N)


@pytest.mark.parametrize("q", [0.5, 0.05, 0.0, 1.0])
def test_impulse_fraction(words, q):
    mask, val = R.impulses(words, int(np.floor(q * 2.0 ** 32)))
    assert abs(float(mask.mean()) - q) <= 5 * np.sqrt(q * (1 - q) / N)
    assert val.dtype == np.float32 and val.min() >= 0 and val.max() < 1 and abs(float(val.mean()) - 0.5) <= 5 / np.sqrt(12 * N)


def test_gamma_mapping_at_both_ends():
    lo, hi = A.gamma_interval((0.8, 1.2))
    assert lo == pytest.approx(-0.25) and hi == pytest.approx(0.2)
    assert A.gamma_exponent(lo) == pytest.approx(0.8) and A.gamma_exponent(hi) == pytest.approx(1.2) and A.gamma_exponent(0.0) == 1.0
    assert A.gamma_interval((1.0, 1.0)) == (0.0, 0.0) and A.gamma_interval((2.0, 0.5)) == (1.0, -1.0)


def test_gaussian_weights_are_scipy_s():
    import scipy.ndimage
    for sigma in (0.5, 0.9, 1.5):
        w = A.gaussian_weights(sigma)
        r = int(4 * sigma + 0.5)
        delta = np.zeros(4 * r + 1)
        delta[2 * r] = 1
        assert w.dtype == np.float32 and w.size == 2 * r + 1
        assert np.allclose(w, scipy.ndimage.gaussian_filter1d(delta, sigma)[r:3 * r + 1], rtol=1e-6, atol=0)
    with pytest.raises(ValueError, match="radius"):
        A.gaussian_weights(1.7)


class Recorder:
    """a numpy Generator that notes every draw"""

    def __init__(self, seed):
        self.rng, self.calls = np.random.default_rng(seed), []

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name,) + tuple(x for x in a if isinstance(x, (int, tuple))))
            return getattr(self.rng, name)(*a, **k)
        return call


ALWAYS = dict(noise_p=1.0, intensity_p=1.0, gamma_p=1.0, impulse_p=1.0, smooth_p=1.0, prob_missing=0.5, prob_low_contrast=0.5)


def test_draw_order():
    d = 6
    rec = Recorder(3)
    plan = A.draw_intensity_plan(rec, A.IntensityParams(**ALWAYS), (d, 8, 8))
    names = [c[0] for c in rec.calls]
    # coin, coin + scale + shift, coin + gamma, coin, coin + sigma, defect r (+ values), seed
    assert names == ["random", "random", "uniform", "uniform", "random", "uniform", "random", "random", "uniform", "random", "random", "integers"], names
    assert plan.applied and plan.noise_sigma == float(np.float32(0.1)) and plan.impulse_threshold == 2 ** 32
    assert plan.scale.shape == plan.shift.shape == plan.gamma.shape == (d,) and plan.scale.dtype == plan.gamma.dtype == np.float32
    assert plan.defect.dtype == np.int32 and set(plan.defect.tolist()) <= {1, 2, 3} and plan.weights.size == 2 * int(4 * plan.blur + 0.5) + 1
    assert 0.9 <= plan.scale.min() and plan.scale.max() <= 1.1 and np.abs(plan.shift).max() <= 0.1 and 0.8 <= plan.gamma.min() and plan.gamma.max() <= 1.2001


def test_a_node_that_is_off_takes_no_draw():
    off = dict(noise_p=0.0, intensity_p=0.0, gamma_p=0.0, impulse_p=0.0, smooth_p=0.0, prob_missing=0.0, prob_low_contrast=0.0)
    rec = Recorder(3)
    plan = A.draw_intensity_plan(rec, A.IntensityParams(**off), (4, 8, 8))
    assert rec.calls == [] and not plan.applied
    for key, draws in (("noise_p", ["random", "integers"]), ("gamma_p", ["random", "uniform"]), ("smooth_p", ["random", "uniform"]),
                       ("impulse_p", ["random", "integers"]), ("intensity_p", ["random", "uniform", "uniform"])):
        rec = Recorder(3)
        A.draw_intensity_plan(rec, A.IntensityParams(**dict(off, **{key: 1.0})), (4, 8, 8))
        assert [c[0] for c in rec.calls] == draws, key
    rec = Recorder(3)
    plan = A.draw_intensity_plan(rec, A.IntensityParams(**dict(off, prob_low_contrast=1.0)), (4, 8, 8))
    assert [c[0] for c in rec.calls] == ["random", "random"] and plan.defect.tolist() == [3, 3, 3, 3]
    # the default of impulse_pixel_p is what the reference executes, impulse_p; the key gives the documented value
    p = A.draw_intensity_plan(np.random.default_rng(0), A.IntensityParams(**dict(off, impulse_p=1.0, impulse_pixel_p=0.05)), (4, 8, 8))
    assert p.impulse_threshold == int(np.floor(0.05 * 2.0 ** 32))
    # a seed for the same stream gives the same plan
    a = A.draw_intensity_plan(np.random.default_rng(9), A.IntensityParams(), (4, 8, 8))
    b = A.draw_intensity_plan(np.random.default_rng(9), A.IntensityParams(), (4, 8, 8))
    assert a.seed == b.seed and a.applied == b.applied and np.array_equal(a.defect, b.defect)


def test_config_key():
    assert A.AugParams.from_config(True).intensity is None
    assert A.AugParams.from_config({"intensity": False}).intensity is None and A.AugParams.from_config({"intensity": False}) == A.AugParams()
    assert A.AugParams.from_config({"intensity": True}).intensity == A.IntensityParams()
    d = A.IntensityParams()
    assert (d.noise_p, d.noise_var, d.intensity_p, d.scale, d.shift, d.gamma_p, d.gamma, d.impulse_p, d.impulse_pixel_p, d.smooth_p, d.blur,
            d.prob_missing, d.prob_low_contrast, d.contrast_scale) == (0.5, 0.01, 0.5, (0.9, 1.1), (-0.1, 0.1), 0.5, (0.8, 1.2), 0.5, None, 0.5,
                                                                      (0.5, 1.5), 0.1, 0.1, 0.1)
    p = A.AugParams.from_config({"simple": False, "deform_p": 0, "shift_p": 0,
                                 "intensity": {"noise_p": 1, "noise_var": 0.04, "scale": [0.8, 1.2], "blur": [1, 1.25], "impulse_pixel_p": 0.05,
                                               "prob_missing": 0.3}})
    assert not p.simple and p.deform_p == 0 and p.intensity == A.IntensityParams(noise_p=1.0, noise_var=0.04, scale=(0.8, 1.2), blur=(1.0, 1.25),
                                                                                 impulse_pixel_p=0.05, prob_missing=0.3)
    with pytest.raises(ValueError, match="unknown augment.intensity key.*clahe"):
        A.AugParams.from_config({"intensity": {"clahe": True}})
    with pytest.raises(ValueError, match="unknown augment key.*noise_p"):
        A.AugParams.from_config({"noise_p": 1})
    with pytest.raises(ValueError, match="probability"):
        A.AugParams.from_config({"intensity": {"gamma_p": 2}})
    with pytest.raises(ValueError, match="blur"):
        A.AugParams.from_config({"intensity": {"blur": [0.5, 2.0]}})
    with pytest.raises(ValueError, match="exceeds 1"):
        A.AugParams.from_config({"intensity": {"prob_missing": 0.6, "prob_low_contrast": 0.6}})
    with pytest.raises(ValueError, match="true, false or a table"):
        A.AugParams.from_config({"intensity": 3})


def test_config_reaches_the_source_and_refusals_stay():
    from bootstrapper_amd.train import make_sample_source
    first = {"input_shape": [8, 32, 32], "output_shape": [4, 16, 16],
             "outputs": {"3d_affs": {"dims": 3, "neighborhood": [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]}}}
    with pytest.raises(ValueError, match="unknown augment.intensity key.*sigma"):
        make_sample_source({"samples": [], "augment": {"intensity": {"sigma": 2}}}, first)
    two_d = {"input_shape": [32, 32], "output_shape": [16, 16], "downsample_factors": [[2, 2]], "outputs": {"2d_affs": {"dims": 2}}}
    with pytest.raises(NotImplementedError, match="2-D"):
        make_sample_source({"samples": [], "augment": {"intensity": True}}, two_d)


@pytest.mark.parametrize("block,nodes", R.CASES)
def test_emulation_passes_the_comparisons(block, nodes):
    shape = R.BLOCKS[block]
    plan, x0, emu = R.build_plan(shape, nodes), R.build_block(shape), R.Emulation()
    R.check(R.staged(emu, x0, plan), plan, emu.chain(x0, plan))


@pytest.mark.parametrize("fault", R.FAULTS)
def test_comparisons_catch_the_fault(fault):
    """each fault is caught, on every block it can show on, by the comparison of its own node"""
    node = {"block_mean": "stats", "gamma_unnormalised": "gamma", "mirror_border": "smooth", "noise_unclipped": "noise",
            "defect_before_smooth": "chain", "impulse_wrong_word": "differs where the rule is exact"}[fault]
    for block, shape in R.BLOCKS.items():
        if fault == "block_mean" and shape[0] == 1:
            continue   # one section: the block's mean is the section's
        plan, x0, emu = R.build_plan(shape, "all"), R.build_block(shape), R.Emulation(fault)
        with pytest.raises(AssertionError, match=node):
            R.check(R.staged(emu, x0, plan), plan, emu.chain(x0, plan), show=lambda s: None)
