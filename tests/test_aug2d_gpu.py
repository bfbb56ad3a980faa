"""The batched augmentation launches of the 2-D setups (csrc/augment2d.hip through bootstrapper_amd/augment2d.py) on their
own inputs, against tests/aug2d_ref.py: S = 3 draws per launch with three different plans -- one of them the identity --
and crops of three shapes, so that a draw reading another's descriptor, lattice, shifts or crop shows.  The coordinate planes
against the float64 map within the derived gate, labels and mask bit for bit against the restatement sampling THE DEVICE'S
OWN planes (no pixel left out), raw against the float64 bilinear on those planes; and exact cases that need no reference."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug2d_ref as R  # noqa: E402
from bootstrapper_amd import augment2d as A  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda(0)


def launch(plans, boxes, crops, regions):
    """-> (coords numpy, [(raw, labels, mask) numpy per region]) of one batch"""
    raw, lab, mask = crops
    p = A.Packed2D(plans, boxes)
    coords = A.coords2d(p, 0)
    raw_d, lab_d, mask_d = dev(p.pack(raw, np.uint8)), dev(p.pack(lab, np.int64)), dev(p.pack(mask, np.uint8))
    outs = []
    for region in regions:
        x = A.sample_raw2d(p, coords, raw_d, region)
        assert x.dtype == torch.float32
        outs.append((x.cpu().numpy(), A.sample_labels2d(p, coords, lab_d, region).cpu().numpy(), A.sample_mask2d(p, coords, mask_d, region).cpu().numpy()))
    return coords.cpu().numpy(), outs


@pytest.mark.parametrize("case", sorted(R.CASES))
@pytest.mark.parametrize("spacing", sorted(R.SPACINGS))
def test_launches_vs_reference(case, spacing):
    plans, boxes, window = R.build_case(case, R.SPACINGS[spacing])
    crops = R.build_crops(boxes, plans[0].sections)
    assert len({tuple(c.shape) for c in crops[1]}) == 3                 # three crop shapes in one launch
    coords, outs = launch(plans, boxes, crops, R.regions(plans, window))
    K = plans[0].sections
    assert coords.shape == (3, K, 2) + plans[0].frame_shape
    assert outs[1][0].shape == (K, 3) + plans[0].shape and outs[2][1].shape == (3,) + window[1]
    res = R.compare(plans, boxes, crops, window, coords, outs)
    print(f"{case} {spacing}: coords largest |device - float64| {res['coords_worst']:.3e}, {res['coords_excess']:.3f} of its gate; "
          f"raw largest |device - float64| {res['raw_err']:.3e} (gate {R.RAW_GATE:.3e})")
    assert res["coords_excess"] <= 1.0, res
    assert res["labels_equal"] and res["mask_equal"]
    assert res["raw_err"] <= R.RAW_GATE


def raw_exact(got, want_u8):
    """float32 output against v * 2 / 255 - 1 in float64, to one float32 ulp at the value"""
    want = want_u8.astype(np.float64) * 2.0 / 255.0 - 1.0
    return bool((np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all())


INP, FRAME, K = (24, 24), ((-2, -2), (26, 26)), 3
BOX = ((-8, -8), (32, 32))     # crops of (40, 40): the input section is [8, 32) of them
SECTION = ((0, 0), INP)


@pytest.fixture(scope="module")
def crops():
    return R.build_crops([BOX] * 3, K, seed=3)


def run(plans, crops):
    _, outs = launch(plans, [BOX] * 3, crops, [SECTION])
    return outs[0]


def centre(a, dy=0, dx=0):
    return a[..., 8 + dy:32 + dy, 8 + dx:32 + dx]


def test_exact_plans_side_by_side(crops):
    """identity, y/x-mirror-only and z-mirror-only plans in ONE launch: slices and flips of each draw's own crop"""
    raw_c, lab_c, mask_c = crops
    plans = [A.Aug2DPlan(INP, FRAME, K), A.Aug2DPlan(INP, FRAME, K, mirror=(False, True, True)), A.Aug2DPlan(INP, FRAME, K, mirror=(True, False, False))]
    raw, lab, mask = run(plans, crops)
    assert np.array_equal(lab[0], centre(lab_c[0])) and np.array_equal(mask[0], centre(mask_c[0])) and raw_exact(raw[:, 0], centre(raw_c[0]))
    assert np.array_equal(lab[1], centre(lab_c[1])[::-1, ::-1]) and np.array_equal(mask[1], centre(mask_c[1])[::-1, ::-1])
    assert raw_exact(raw[:, 1], centre(raw_c[1])[:, ::-1, ::-1])
    # the z mirror reverses the sections of raw and leaves the planes alone; z is never interpolated
    assert np.array_equal(lab[2], centre(lab_c[2])) and raw_exact(raw[:, 2], centre(raw_c[2])[::-1])


def test_swap_and_single_mirrors(crops):
    raw_c, lab_c, mask_c = crops
    plans = [A.Aug2DPlan(INP, FRAME, K, swap=True), A.Aug2DPlan(INP, FRAME, K, mirror=(False, True, False)),
             A.Aug2DPlan(INP, FRAME, K, swap=True, mirror=(False, True, False))]
    raw, lab, mask = run(plans, crops)
    assert np.array_equal(lab[0], centre(lab_c[0]).T) and raw_exact(raw[:, 0], centre(raw_c[0]).transpose(0, 2, 1))
    assert np.array_equal(lab[1], centre(lab_c[1])[::-1]) and np.array_equal(mask[1], centre(mask_c[1])[::-1])
    # swap and mirror together: the swap comes first, then the mirror acts on the output axis
    assert np.array_equal(lab[2], centre(lab_c[2])[::-1, :].T)


def test_integer_shift_only_plans_shift_each_section(crops):
    """labels and mask take the shift of section K // 2, raw's section k its own; draw 1 has no shift between two that have"""
    raw_c, lab_c, mask_c = crops
    sh = [np.array([[0, 3, -8], [-7, 8, 2]], dtype=np.int32), None, np.array([[8, -8, 1], [5, 0, -8]], dtype=np.int32)]
    raw, lab, mask = run([A.Aug2DPlan(INP, FRAME, K, shifts=s) for s in sh], crops)
    for s in range(3):
        z = np.zeros((2, K), dtype=np.int32) if sh[s] is None else sh[s]
        assert np.array_equal(lab[s], centre(lab_c[s], z[0, 1], z[1, 1])) and np.array_equal(mask[s], centre(mask_c[s], z[0, 1], z[1, 1]))
        for k in range(K):
            assert raw_exact(raw[k, s], centre(raw_c[s][k], z[0, k], z[1, k]))


def test_odd_section_without_swap():
    """(17, 33): the width is odd and no multiple of a wave or a vector; mirrored about (I - 1) / 2 = 16 exactly"""
    inp = (17, 33)
    boxes = [((0, 0), inp)] * 3
    raw_c, lab_c, _ = crops3 = R.build_crops(boxes, 1, seed=4)
    plans = [A.Aug2DPlan(inp, None, 1, mirror=(False, False, True)), A.Aug2DPlan(inp, None, 1), A.Aug2DPlan(inp, None, 1, mirror=(False, True, False))]
    _, outs = launch(plans, boxes, crops3, [None])
    raw, lab, _ = outs[0]
    assert np.array_equal(lab[0], lab_c[0][:, ::-1]) and np.array_equal(lab[1], lab_c[1]) and np.array_equal(lab[2], lab_c[2][::-1])
    assert raw_exact(raw[0, 0], raw_c[0][0][:, ::-1]) and raw_exact(raw[0, 2], raw_c[2][0][::-1])


def test_refusals():
    from bootstrapper_amd import _lib

    def invalid(match, fn):
        with pytest.raises(_lib.BsmiError, match=match) as e:
            fn()
        assert e.value.code == _lib.ERR_INVALID
    box = ((0, 0), (17, 33))
    invalid("square", lambda: A.coords2d(A.Packed2D([A.Aug2DPlan((17, 33), None, 1, swap=True)], [box]), 0))
    ones = np.ones(2, dtype=np.float32)
    big = A.Aug2DPlan((16, 16), None, 1, lattice=np.zeros((2, 65, 64), dtype=np.float32), inv_spacing=ones)
    invalid("4096", lambda: A.coords2d(A.Packed2D([A.Aug2DPlan((16, 16), None, 1), big], [((0, 0), (16, 16))] * 2), 0))
    ok = A.Packed2D([A.Aug2DPlan((16, 16), None, 1, lattice=np.zeros((2, 64, 64), dtype=np.float32), inv_spacing=ones)], [((0, 0), (16, 16))])
    coords = A.coords2d(ok, 0)
    lab = torch.zeros(256, dtype=torch.int64, device="cuda:0")
    invalid("leaves the frame", lambda: A.sample_labels2d(ok, coords, lab, ((1, 0), (16, 16))))
    # S < 1, K < 1, a crop beyond the packed crops, 2^31 elements or more: the C entry points themselves
    import ctypes as C
    i2 = lambda a, b: (C.c_int64 * 2)(a, b)  # noqa: E731
    tab, ptr, st = ok.draws, C.c_void_p(ok.dev[0].data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cp, lp, shape = C.c_void_p(coords.data_ptr()), C.c_void_p(lab.data_ptr()), i2(16, 16)
    lat = C.c_void_p(ok.dev[1].data_ptr())
    invalid("at least 1", lambda: _lib.check(_lib.lib.bsmi_aug2d_coords(0, tab, ptr, 0, 1, shape, i2(0, 0), shape, None, lat, 8192, cp, st)))
    invalid("at least 1", lambda: _lib.check(_lib.lib.bsmi_aug2d_coords(0, tab, ptr, 1, 0, shape, i2(0, 0), shape, None, lat, 8192, cp, st)))
    invalid("leaves the packed lattice", lambda: _lib.check(_lib.lib.bsmi_aug2d_coords(0, tab, ptr, 1, 1, shape, i2(0, 0), shape, None, lat, 8191, cp, st)))
    invalid("2\\^31", lambda: _lib.check(_lib.lib.bsmi_aug2d_coords(0, tab, ptr, 1, 1, shape, i2(0, 0), i2(1 << 15, 1 << 15), None, lat, 8192, cp, st)))
    invalid("does not contain the input", lambda: _lib.check(_lib.lib.bsmi_aug2d_coords(0, tab, ptr, 1, 1, shape, i2(1, 0), shape, None, lat, 8192, cp, st)))
    invalid("leaves the packed crops", lambda: _lib.check(_lib.lib.bsmi_aug2d_sample_nearest_i64(0, tab, ptr, 1, 1, cp, shape, i2(0, 0), shape, lp, 255, lp, st)))
    invalid("at least 1", lambda: _lib.check(_lib.lib.bsmi_aug2d_sample_nearest_i64(0, tab, ptr, 0, 1, cp, shape, i2(0, 0), shape, lp, 256, lp, st)))
    torch.cuda.synchronize()
