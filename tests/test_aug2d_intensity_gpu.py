"""The batched intensity launches of the 2-D setups (csrc/augment2d_intensity.hip through bootstrapper_amd/augment2d.py) on
their own inputs: S draws per launch with different plans -- one applies every node, one is untouched, one is smooth-only or a
single other node -- so that a draw reading another's descriptor, row, taps or sections shows.  The contract is bit-equality
with the 3-D chain (augment.apply_intensity on each draw's stack, which tests/test_intensity_gpu.py holds to float64): the
arithmetic is the same device code, so no tolerance is involved; one float64 check per case through intensity_ref.check on
each draw's stack, with its gates, every node through its batched entry."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug2d_intensity_ref as R2  # noqa: E402
import aug2d_ref  # noqa: E402
from bootstrapper_amd import augment as G  # noqa: E402
from bootstrapper_amd import augment2d as A  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda(0)


class Device:
    """the backend `nodes` of aug2d_intensity_ref.compare: every batched launch through its own wrapper, numpy in, numpy out"""

    def __init__(self, ipacked):
        self.t = ipacked

    def stats(self, b):
        return A.plane_stats(dev(b)).cpu().numpy()

    def noise(self, b):
        return A.noise2d(dev(b), self.t).cpu().numpy()

    def impulse(self, b):
        return A.impulse2d(dev(b), self.t).cpu().numpy()

    def smooth(self, b):
        return A.smooth2d(dev(b), self.t).cpu().numpy()

    def intensity(self, b, st):
        return A.intensity2d(dev(b), self.t, dev(st)).cpu().numpy()

    def gamma(self, b, st):
        return A.gamma2d(dev(b), self.t, dev(st)).cpu().numpy()

    def defect(self, b, st, final_map):
        return A.defect2d(dev(b), self.t, dev(st) if st is not None else None, final_map).cpu().numpy()

    def chain(self, b, final_map):
        return A.apply_intensity2d(dev(b), self.t, final_map).cpu().numpy()


class Block:
    """`block` of compare: the 3-D launches of csrc/augment_intensity.hip on one draw's stack"""

    def chain(self, stack, plan, final_map):
        return G.apply_intensity(dev(stack), plan, final_map).cpu().numpy()

    def node(self, name, stack, plan, st):
        x, st = dev(stack), dev(st)
        return {"noise": lambda: G.noise(x, plan.seed, plan.noise_sigma), "intensity": lambda: G.intensity(x, st, plan.scale, plan.shift),
                "gamma": lambda: G.gamma(x, st, plan.gamma), "impulse": lambda: G.impulse(x, plan.seed, plan.impulse_threshold),
                "smooth": lambda: G.smooth(x, plan.weights), "defect": lambda: G.defect(x, st, plan.defect, plan.contrast_scale)}[name]().cpu().numpy()


@pytest.mark.parametrize("case", sorted(R2.CASES))
def test_batched_chain_is_the_3d_chain_of_every_draw(case):
    """checks 1, 2 and 4: bit-equality with the 3-D chain after the whole chain and after each single node, untouched draws and
    draws without a node bit-equal to their input, two runs bit-equal, and the float64 comparison of every launch"""
    x, plans = R2.build_case(case)
    R2.compare(Device(A.PackedIntensity2D(plans)), x, plans, Block())
    # the plane statistics are the 3-D section statistics of every stack, bit for bit (one reduction order)
    st = A.plane_stats(dev(x)).cpu().numpy().reshape(x.shape[0], x.shape[1], 3)
    for s in range(x.shape[1]):
        assert np.array_equal(st[:, s], G.section_stats(dev(x[:, s])).cpu().numpy())


@pytest.mark.parametrize("case", sorted(aug2d_ref.CASES))
def test_unit_resampling(case):
    """bsmi_aug2d_sample_unit_f32_u8: touched draws against the float64 bilinear value on the device's own coordinates divided
    by 255, untouched draws bit-equal to bsmi_aug2d_sample_f32_u8 on the same tables.

    The gate, derived as aug2d_ref derives RAW_GATE (eps = 2^-24, first order, times 1 + 2^-10): two lerp levels on values of at
    most 255 cost 10 eps 255, which the division by 255 carries into output units as 10 eps; the division itself is one
    relative rounding of a result of at most 1: 1 eps.  UNIT_GATE = 11 eps (1 + 2^-10), half the raw gate of 22 eps: one
    operation fewer (no v * 2 - 255) and half the magnitude."""
    unit_gate = 11 * aug2d_ref.EPS * aug2d_ref.SLACK
    assert unit_gate <= aug2d_ref.RAW_GATE
    plans, boxes, window = aug2d_ref.build_case(case, aug2d_ref.SPACINGS["spacing4"])
    raw_c = aug2d_ref.build_crops(boxes, plans[0].sections)[0]
    K, shape = plans[0].sections, (plans[0].sections,) + plans[0].shape
    # draw 1, the identity of the geometric case, is the touched one here; then the other way round
    for touched in ([False, True, False], [True, False, True]):
        iplans = [G.IntensityPlan(shape, impulse_threshold=1, seed=1) if t else G.IntensityPlan(shape) for t in touched]
        ip = A.PackedIntensity2D(iplans)
        assert ip.touched == touched
        p = A.Packed2D(plans, boxes)
        coords = A.coords2d(p, 0)
        crops = dev(p.pack(raw_c, np.uint8))
        for region in aug2d_ref.regions(plans, window):
            unit = A.sample_unit2d(p, coords, crops, ip, region).cpu().numpy()
            final = A.sample_raw2d(p, coords, crops, region).cpu().numpy()
            c = coords.cpu().numpy()
            for s, plan in enumerate(plans):
                if not touched[s]:
                    assert np.array_equal(unit[:, s], final[:, s]), f"draw {s}: an untouched draw differs from sample_raw2d"
                    continue
                want = np.stack([aug2d_ref.bilinear_f64(aug2d_ref._window(c[s, k], plan, region), raw_c[s][K - 1 - k if plan.mirror[0] else k]) / 255.0
                                 for k in range(K)])
                err = float(np.abs(unit[:, s].astype(np.float64) - want).max())
                print(f"{case} draw {s}: unit raw largest |device - float64| {err:.3e} (gate {unit_gate:.3e})")
                assert err <= unit_gate
                assert unit[:, s].min() >= 0.0 and unit[:, s].max() <= 1.0


def test_refusals():
    """every BSMI_ERR_INVALID case is the host-side check's: the tables in host memory are read, nothing is launched"""
    from bootstrapper_amd import _lib
    x, plans = R2.build_case("S3_K3_24x24")
    S, K, H, W = 3, 3, 24, 24
    t = A.PackedIntensity2D(plans)
    xd = dev(x)
    before = xd.clone()
    table, planes, taps = t.upload(xd.device)
    st = A.plane_stats(xd)
    L = _lib.lib
    tp, xp, sp, strm = C.c_void_p(table.data_ptr()), C.c_void_p(xd.data_ptr()), C.c_void_p(st.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tmp = torch.empty_like(xd)
    mp, wp = C.c_void_p(tmp.data_ptr()), C.c_void_p(taps.data_ptr())
    i2 = lambda a, b: (C.c_int64 * 2)(a, b)  # noqa: E731
    shape = i2(H, W)
    modes = t.planes[3].ctypes.data_as(C.POINTER(C.c_int32))
    row = lambda r: C.c_void_p(planes[r].data_ptr())  # noqa: E731

    def invalid(match, fn):
        with pytest.raises(_lib.BsmiError, match=match) as e:
            _lib.check(fn())
        assert e.value.code == _lib.ERR_INVALID

    invalid("at least 1", lambda: L.bsmi_aug2d_noise_f32(0, t.idraws, tp, 0, K, shape, xp, strm))
    invalid("at least 1", lambda: L.bsmi_aug2d_noise_f32(0, t.idraws, tp, S, 0, shape, xp, strm))
    invalid("at least 1", lambda: L.bsmi_aug2d_defect_f32(0, t.idraws, tp, 0, K, shape, xp, sp, modes, row(3), 1, strm))
    invalid("2\\^31", lambda: L.bsmi_aug2d_impulse_f32(0, t.idraws, tp, S, K, i2(1 << 14, 1 << 14), xp, strm))   # 9 * 2^28
    invalid("2\\^31", lambda: L.bsmi_aug2d_smooth_f32(0, t.idraws, tp, S, K, i2(1 << 14, 1 << 14), xp, mp, wp, int(taps.numel()), strm))
    invalid("leave the packed taps", lambda: L.bsmi_aug2d_smooth_f32(0, t.idraws, tp, S, K, shape, xp, mp, wp, int(taps.numel()) - 1, strm))
    t.idraws[0].radius = 7
    invalid("radius", lambda: L.bsmi_aug2d_smooth_f32(0, t.idraws, tp, S, K, shape, xp, mp, wp, int(taps.numel()), strm))
    invalid("radius", lambda: L.bsmi_aug2d_noise_f32(0, t.idraws, tp, S, K, shape, xp, strm))
    t.idraws[0].radius = 6
    t.idraws[2].taps_offset = -1
    invalid("leave the packed taps", lambda: L.bsmi_aug2d_smooth_f32(0, t.idraws, tp, S, K, shape, xp, mp, wp, int(taps.numel()), strm))
    t.idraws[2].taps_offset = 13
    t.planes[3, 0] = 4                                                          # plane 0: section 0 of draw 0, which has the defect node
    invalid("defect mode 4", lambda: L.bsmi_aug2d_defect_f32(0, t.idraws, tp, S, K, shape, xp, sp, modes, row(3), 1, strm))
    t.planes[3, 0] = -1
    invalid("defect mode -1", lambda: L.bsmi_aug2d_defect_f32(0, t.idraws, tp, S, K, shape, xp, sp, modes, row(3), 1, strm))
    t.planes[3, 0] = 3
    t.idraws[1].nodes = 128
    invalid("mask of bits", lambda: L.bsmi_aug2d_gamma_f32(0, t.idraws, tp, S, K, shape, xp, sp, row(2), strm))
    t.idraws[1].nodes = 0
    invalid("null descriptor table", lambda: L.bsmi_aug2d_noise_f32(0, None, tp, S, K, shape, xp, strm))
    with pytest.raises(ValueError, match="contiguous float32"):
        A.noise2d(xd[:, :2], t)
    with pytest.raises(ValueError, match="plane_stats"):
        A.gamma2d(xd, t, st[:3])
    torch.cuda.synchronize()
    assert torch.equal(xd, before)                                              # nothing ran
