"""The launches of the input augmentation of the second-stage setups (csrc/augment_inputs.hip through
bootstrapper_amd/augment_inputs.py), each on its own input against tests/augin_ref.py: the array before a launch is read back and
goes through the float64 rule, the array after it is compared with that -- radius-0 sections, untouched sections and skipped
nodes bit for bit, the others within their gates."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augin_ref as R  # noqa: E402
from bootstrapper_amd import augment_inputs as A  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda(0)


class Device:
    """the backend of R.staged: every node through its own wrapper, numpy in, numpy out"""

    def noise(self, x, seed, sigma):
        return A.noise(dev(x), seed, sigma).cpu().numpy()

    def group_mean(self, x, axis):
        return A.group_mean(dev(x), axis).cpu().numpy()

    def intensity(self, x, mean, scale, shift, axis):
        return A.intensity(dev(x), dev(mean), scale, shift, axis).cpu().numpy()

    def smooth(self, x, weights, radius, channels):
        return A.smooth(dev(x), weights, radius, channels).cpu().numpy()

    def contrast(self, x, mean, mode, contrast_scale):
        return A.contrast(dev(x), dev(mean), mode, contrast_scale).cpu().numpy()

    def chain(self, x, plan):
        return A.apply_inputs(dev(x), plan).cpu().numpy()


@pytest.mark.parametrize("array,nodes", R.CASES)
def test_launches_vs_reference(array, nodes):
    shape = R.ARRAYS[array]
    plan, x0, ops = R.build_plan(shape, nodes), R.build_array(shape), Device()
    chain = ops.chain(x0, plan)
    rec = R.staged(ops, x0, plan)
    seen = R.check(rec, plan, chain)
    print(f"observed {array} {nodes}: " + ", ".join(f"{k} {v:.3e}" for k, v in seen.items()))
    assert np.array_equal(ops.chain(x0, plan), chain)                                   # two runs of one plan
    assert chain.min() >= 0.0 and chain.max() <= 1.0
    for node, before, after, _ in rec:
        if node == "smooth":
            still = plan.radius == 0
            assert np.array_equal(after[:, still], before[:, still])                    # a section of radius 0: bit for bit
        if node == "contrast":
            still = plan.low_contrast != 3
            assert np.array_equal(after[:, still], before[:, still])


def test_skipped_nodes_leave_the_array_bit_equal():
    shape = R.ARRAYS["3x4x20x20"]
    x0 = R.build_array(shape)
    empty = A.InputPlan(shape)
    assert not empty.applied
    assert np.array_equal(A.apply_inputs(dev(x0), empty).cpu().numpy(), x0)
    assert np.array_equal(A.contrast(dev(x0), A.group_mean(dev(x0), 1), np.zeros(4, dtype=np.int32), 0.1).cpu().numpy(), x0)
    weights, radius = A.section_taps([0.1, 0.12, 0.1, 0.11])                            # radius 0 everywhere
    assert np.array_equal(A.smooth(dev(x0), weights, radius).cpu().numpy(), x0)
    assert np.array_equal(A.smooth(dev(x0), weights, radius, channels=False).cpu().numpy(), x0)
    assert np.array_equal(A.noise(dev(x0), 5, 0.0).cpu().numpy(), x0)                   # sigma 0 adds 0 to values in [0, 1]
    ones, zeros = np.ones(3, dtype=np.float32), np.zeros(3, dtype=np.float32)           # scale 1, shift 0 on means that are exact
    flat = np.full(shape, 0.25, dtype=np.float32)
    assert np.array_equal(A.intensity(dev(flat), A.group_mean(dev(flat), 0), ones, zeros, 0).cpu().numpy(), flat)


def test_every_channel_has_its_own_noise():
    """the counter is the linear index within the array: channel c of the array is section block c of the 3-D chain's noise"""
    from bootstrapper_amd import augment
    shape = R.ARRAYS["6x3x24x40"]
    x0 = np.full(shape, 0.5, dtype=np.float32)
    y = A.noise(dev(x0), 11, 0.1).cpu().numpy()
    assert np.array_equal(y, augment.noise(dev(x0.reshape(18, 24, 40)), 11, 0.1).cpu().numpy().reshape(shape))
    assert not np.array_equal(y[0], y[1])


def test_smoothing_of_ones_stays_in_range():
    """a region of exact ones, as the affinity inputs hold them: float32 taps may add up to 1 and a few ulp, the result may not"""
    shape = (2, 6, 20, 70)
    x0 = np.ones(shape, dtype=np.float32)
    weights, radius = A.section_taps(np.linspace(0.2, 1.5, 6))
    for channels in (True, False):
        y = A.smooth(dev(x0), weights, radius, channels).cpu().numpy()
        assert y.max() <= 1.0 and y.min() >= 1.0 - 3 * R.SMOOTH_GATE


def test_refusals():
    from bootstrapper_amd import _lib
    x = dev(R.build_array((3, 4, 20, 20)))
    weights, radius = A.section_taps([0.5] * 4)
    with pytest.raises(ValueError, match="radius"):
        A.smooth(x, weights, np.array([2, 7, 2, 2], dtype=np.int32))
    with pytest.raises(ValueError, match="weights"):
        A.smooth(x, weights[:, :5], radius)
    wide = dev(np.zeros((17, 1, 8, 8), dtype=np.float32))
    w1, r1 = A.section_taps([0.5])
    with pytest.raises(ValueError, match="at most 16"):
        A.smooth(wide, w1, r1)
    with pytest.raises(_lib.BsmiError, match="at most 16") as e:                        # the library's own refusal
        tmp, wd, rd = torch.empty_like(wide), dev(w1), dev(r1)
        _lib.check(_lib.lib.bsmi_augin_smooth_f32(0, _lib.i64x4(wide.shape), wide.data_ptr(), tmp.data_ptr(), wd.data_ptr(), rd.data_ptr(), 1, None))
    assert e.value.code == _lib.ERR_INVALID
    assert np.array_equal(A.smooth(wide, w1, r1, channels=False).cpu().numpy(), np.zeros((17, 1, 8, 8), dtype=np.float32))   # no column held
    with pytest.raises(ValueError, match="axis"):
        A.group_mean(x, 2)
    with pytest.raises(ValueError, match="shape"):
        A.intensity(x, A.group_mean(x, 0), np.ones(4, dtype=np.float32), np.zeros(4, dtype=np.float32), 0)
    with pytest.raises(ValueError, match="contiguous float32"):
        A.noise(x.double(), 1, 0.1)
    with pytest.raises(ValueError, match="plan of"):
        A.apply_inputs(x, A.InputPlan((3, 4, 20, 21)))
    torch.cuda.synchronize()
