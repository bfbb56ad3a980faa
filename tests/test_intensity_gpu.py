"""The launches of the intensity augmentation (csrc/augment_intensity.hip through bootstrapper_amd/augment.py), each on its own
input against tests/intensity_ref.py: the block before a launch is read back and goes through the float64 rule, the block
after it is compared with that -- impulses, missing sections and skipped nodes bit for bit, the others within their gates."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import intensity_ref as R  # noqa: E402
from bootstrapper_amd import augment as A  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda(0)


class Device:
    """the backend of R.staged: every node through its own wrapper, numpy in, numpy out"""

    def noise(self, x, seed, sigma):
        return A.noise(dev(x), seed, sigma).cpu().numpy()

    def stats(self, x):
        return A.section_stats(dev(x)).cpu().numpy()

    def intensity(self, x, st, scale, shift):
        return A.intensity(dev(x), dev(st), scale, shift).cpu().numpy()

    def gamma(self, x, st, g):
        return A.gamma(dev(x), dev(st), g).cpu().numpy()

    def impulse(self, x, seed, threshold):
        return A.impulse(dev(x), seed, threshold).cpu().numpy()

    def smooth(self, x, weights):
        return A.smooth(dev(x), weights).cpu().numpy()

    def defect(self, x, st, mode, contrast_scale):
        return A.defect(dev(x), dev(st) if st is not None else A._no_stats(dev(x)), mode, contrast_scale).cpu().numpy()

    def chain(self, x, plan):
        return A.apply_intensity(dev(x), plan, final_map=False).cpu().numpy()


@pytest.mark.parametrize("block,nodes", R.CASES)
def test_launches_vs_reference(block, nodes):
    shape = R.BLOCKS[block]
    plan, x0, ops = R.build_plan(shape, nodes), R.build_block(shape), Device()
    chain = ops.chain(x0, plan)
    seen = R.check(R.staged(ops, x0, plan), plan, chain)
    print(f"observed {block} {nodes}: " + ", ".join(f"{k} {v:.3e}" for k, v in seen.items()))
    assert np.array_equal(ops.chain(x0, plan), chain)                                   # two runs of one plan
    final = A.apply_intensity(dev(x0), plan).cpu().numpy()
    assert np.array_equal(final, np.float32(2) * chain - np.float32(1))                 # 2 x is exact: one rounding on either side
    assert final.min() >= -1.0 and final.max() <= 1.0
    if plan.defect is not None:
        for z, md in enumerate(plan.defect):
            if md in (1, 2):
                assert (chain[z] == md - 1).all()                                       # a missing section is exactly 0 or 1


def test_skipped_nodes_leave_the_block_bit_equal():
    shape = R.BLOCKS["3x17x33"]
    x0 = R.build_block(shape)
    empty = A.IntensityPlan(shape)
    assert not empty.applied
    assert np.array_equal(A.apply_intensity(dev(x0), empty, final_map=False).cpu().numpy(), x0)
    assert np.array_equal(A.defect(dev(x0), A._no_stats(dev(x0)), np.zeros(3, dtype=np.int32), 0.1).cpu().numpy(), x0)
    assert np.array_equal(A.impulse(dev(x0), 5, 0).cpu().numpy(), x0)                   # threshold 0: no voxel
    every = A.impulse(dev(x0), 5, 2 ** 32).cpu().numpy()                                # q = 1: every voxel
    assert np.array_equal(every, R.impulses(R.philox(np.arange(x0.size), 5), 2 ** 32)[1].reshape(shape))
    flat = np.full(shape, 0.25, dtype=np.float32)                                       # gamma on sections without range
    assert np.array_equal(A.gamma(dev(flat), A.section_stats(dev(flat)), np.full(3, 1.2, dtype=np.float32)).cpu().numpy(), flat)
    assert np.array_equal(A.noise(dev(x0), 5, 0.0).cpu().numpy(), x0)                   # sigma 0 adds 0 to values in [0, 1]


def test_unit_resampling_and_the_fused_entry():
    """sample_unit is sample_raw's trilinear expression written v / 255; a plan without an applied node goes through sample_raw itself"""
    import aug_ref
    shape = (3, 17, 33)
    raw = aug_ref.build_crops(shape, seed=4)[0]
    coords = A.coords(A.AugPlan(shape, mirror=(False, False, True)), (0, 0, 0), 0)
    unit = A.sample_unit(coords, dev(raw)).cpu().numpy()
    want = raw[:, :, ::-1].astype(np.float64) / 255.0                                    # on voxel centres: one rounded division
    assert (np.abs(unit - want) <= np.spacing(want.astype(np.float32)) / 2).all()
    plan = aug_ref.build_plan(shape, 4.0, seed=11)
    lo, hi = A.source_box(plan)
    raw = aug_ref.build_crops(tuple(h - l for l, h in zip(lo, hi)), seed=12)[0]
    coords = A.coords(plan, lo, 0)
    err = float(np.abs(A.sample_unit(coords, dev(raw)).cpu().numpy() - aug_ref.trilinear_f64(coords.cpu().numpy(), raw) / 255.0).max())
    print(f"unit raw: largest |device - float64| {err:.3e} (gate {aug_ref.RAW_GATE / 2:.3e})")
    assert err <= aug_ref.RAW_GATE / 2                                                   # aug_ref's bound in units of [0, 1]: 15 eps + 1 eps
    assert torch.equal(A.sample_raw_intensity(coords, dev(raw), A.IntensityPlan(plan.shape)), A.sample_raw(coords, dev(raw)))
    assert torch.equal(A.sample_raw_intensity(coords, dev(raw), None), A.sample_raw(coords, dev(raw)))


def test_refusals():
    from bootstrapper_amd import _lib
    x = dev(R.build_block((3, 17, 33)))
    with pytest.raises(_lib.BsmiError, match="radius") as e:
        A.smooth(x, np.full(15, 1 / 15, dtype=np.float32))
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.BsmiError, match="threshold"):
        A.impulse(x, 1, 2 ** 32 + 1)
    with pytest.raises(ValueError, match="per section"):
        A.gamma(x, A.section_stats(x), np.ones(4, dtype=np.float32))
    with pytest.raises(ValueError, match="contiguous float32"):
        A.noise(x.double(), 1, 0.1)
    torch.cuda.synchronize()
