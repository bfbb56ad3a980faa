"""The augmentation launches (csrc/augment.hip through bootstrapper_amd/augment.py) on their own inputs, against
tests/aug_ref.py: the coordinate planes against the float64 map within the derived gate, labels and mask bit for bit against
the reference sampling THE DEVICE'S OWN planes (no voxel left out), raw against the float64 trilinear on those planes; and
exact cases that need no reference at all."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_ref as R  # noqa: E402
from bootstrapper_amd import augment as A  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda(0)


@pytest.mark.parametrize("block", sorted(R.BLOCKS))
@pytest.mark.parametrize("spacing", sorted(R.SPACINGS))
def test_launches_vs_reference(block, spacing):
    shape = R.BLOCKS[block]
    plan = R.build_plan(shape, R.SPACINGS[spacing], seed=11)
    if block == "5x24x24":
        lo, size = (-2, -8, -8), (9, 40, 40)   # smaller than the map's range: the clamp of the sampling kernels works
    else:
        lo, hi = A.source_box(plan)
        size = tuple(h - l for l, h in zip(lo, hi))
    raw, labels, mask = R.build_crops(size, seed=12)
    coords = A.coords(plan, lo, 0)
    got = coords.cpu().numpy()
    excess, worst = R.coords_excess(got, plan, lo)
    print(f"coords {block} {spacing}: largest |device - float64| {worst:.3e}, {excess:.3f} of its gate")
    assert excess <= 1.0, (excess, worst)
    ctx = tuple(min(n // 4, 4) for n in shape)
    regions = [None, (ctx, tuple(n - 2 * c for n, c in zip(shape, ctx))), ((0, 1, 3), (1, shape[1] - 1, shape[2] - 4))]
    for region in regions:
        assert np.array_equal(A.sample_labels(coords, dev(labels), region).cpu().numpy(), R.sample_nearest(got, labels, region))
        assert np.array_equal(A.sample_mask(coords, dev(mask), region).cpu().numpy(), R.sample_nearest(got, mask, region))
        x = A.sample_raw(coords, dev(raw), region)
        assert x.dtype == torch.float32
        err = float(np.abs(x.cpu().numpy().astype(np.float64) - R.sample_raw(got, raw, region)).max())
        print(f"raw {block} {spacing}: largest |device - float64| {err:.3e} (gate {R.RAW_GATE:.3e})")
        assert err <= R.RAW_GATE


def raw_exact(got, want_u8):
    """float32 output against v * 2 / 255 - 1 in float64, to one float32 ulp at the value"""
    want = want_u8.astype(np.float64) * 2.0 / 255.0 - 1.0
    return bool((np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all())


@pytest.fixture(scope="module")
def crops():
    return R.build_crops((9, 40, 40), seed=3)


def run(plan, crops, lo=(-2, -8, -8)):
    raw, labels, mask = crops
    coords = A.coords(plan, lo, 0)
    return (A.sample_raw(coords, dev(raw)).cpu().numpy(), A.sample_labels(coords, dev(labels)).cpu().numpy(),
            A.sample_mask(coords, dev(mask)).cpu().numpy())


def test_identity_plan_returns_the_centre_crop(crops):
    x, lab, m = run(A.AugPlan((5, 24, 24)), crops)
    centre = tuple(slice(a, a + n) for a, n in zip((2, 8, 8), (5, 24, 24)))
    assert np.array_equal(lab, crops[1][centre]) and np.array_equal(m, crops[2][centre]) and raw_exact(x, crops[0][centre])


@pytest.mark.parametrize("mirror", [(True, False, False), (False, True, False), (False, False, True), (True, True, True)])
def test_mirror_only_plans_are_flips(crops, mirror):
    x, lab, m = run(A.AugPlan((5, 24, 24), mirror=mirror), crops)
    flip = tuple(slice(None, None, -1) if f else slice(None) for f in mirror)
    centre = tuple(slice(a, a + n) for a, n in zip((2, 8, 8), (5, 24, 24)))
    assert np.array_equal(lab, crops[1][centre][flip]) and np.array_equal(m, crops[2][centre][flip]) and raw_exact(x, crops[0][centre][flip])


def test_swap_only_plan_is_a_transpose(crops):
    x, lab, m = run(A.AugPlan((5, 24, 24), swap=True), crops)
    centre = tuple(slice(a, a + n) for a, n in zip((2, 8, 8), (5, 24, 24)))
    assert np.array_equal(lab, crops[1][centre].transpose(0, 2, 1)) and raw_exact(x, crops[0][centre].transpose(0, 2, 1))
    # swap and mirrors together: the swap comes first, then the mirrors act on the output axes
    x, lab, m = run(A.AugPlan((5, 24, 24), swap=True, mirror=(False, True, False)), crops)
    assert np.array_equal(lab, crops[1][centre][:, ::-1, :].transpose(0, 2, 1))


def test_integer_shift_only_plan_shifts_each_section(crops):
    shifts = np.array([[0, 3, -8, 8, 1], [-7, 0, 8, -2, -8]], dtype=np.int32)
    x, lab, m = run(A.AugPlan((5, 24, 24), shifts=shifts), crops)
    for z in range(5):
        sl = (2 + z, slice(8 + shifts[0, z], 32 + shifts[0, z]), slice(8 + shifts[1, z], 32 + shifts[1, z]))
        assert np.array_equal(lab[z], crops[1][sl]) and np.array_equal(m[z], crops[2][sl]) and raw_exact(x[z], crops[0][sl])


def test_odd_block_without_swap(crops):
    """(3, 17, 33): the width is odd and no multiple of a wave or a vector; mirrored about (I - 1) / 2 = 16 exactly"""
    raw, labels, mask = R.build_crops((3, 17, 33), seed=4)
    coords = A.coords(A.AugPlan((3, 17, 33), mirror=(False, False, True)), (0, 0, 0), 0)
    assert np.array_equal(A.sample_labels(coords, dev(labels)).cpu().numpy(), labels[:, :, ::-1])
    assert raw_exact(A.sample_raw(coords, dev(raw)).cpu().numpy(), raw[:, :, ::-1])


def test_refusals():
    from bootstrapper_amd import _lib
    plan = A.AugPlan((3, 17, 33), swap=True)
    with pytest.raises(_lib.BsmiError, match="square") as e:
        A.coords(plan, (0, 0, 0), 0)
    assert e.value.code == _lib.ERR_INVALID
    big = A.AugPlan((4, 16, 16), lattice=np.zeros((3, 17, 16, 16), dtype=np.float32), inv_spacing=np.ones(3, dtype=np.float32))
    with pytest.raises(_lib.BsmiError, match="4096") as e:
        A.coords(big, (0, 0, 0), 0)
    assert e.value.code == _lib.ERR_INVALID
    A.coords(A.AugPlan((4, 16, 16), lattice=np.zeros((3, 16, 16, 16), dtype=np.float32), inv_spacing=np.ones(3, dtype=np.float32)), (0, 0, 0), 0)
    coords = A.coords(A.AugPlan((4, 16, 16)), (0, 0, 0), 0)
    with pytest.raises(_lib.BsmiError, match="leaves the coordinate volume"):
        A.sample_labels(coords, torch.zeros((4, 16, 16), dtype=torch.int64, device="cuda:0"), ((1, 0, 0), (4, 16, 16)))
    torch.cuda.synchronize()
