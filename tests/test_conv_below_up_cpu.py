"""Convolving below the upsampling (csrc/unet_plan_wino.hip WinoStage::below_up, csrc/wino.hip wino4_out_kernel<.., BELOW>), restated
in float64 with the output transform's index contract.  Needs no GPU.

For U = up(1,2,2)(L) (torch's trilinear upsampling, align_corners = False) and a 3x3x3 kernel W,

    conv3d(crop(U))[z, y, x, n] = sum_{ky,kx} up(Y_(ky,kx))[z, oy + y + ky, ox + x + kx, n]
    Y_(ky,kx)[z, i, j, n]       = sum_{kz,c} W[n, c, kz, ky, kx] L[oz + z + kz, i, j, c]

because the interpolation weights do not depend on the channel.  The contract of WinoOutArgs::below: tap t = 3 ky + kx lives
at t * btap + ((z * lH + i) * lW + j) * brow + n of one flat f32 buffer (batched layout: btap = rows * Cpad, brow = Cpad; dense
layout: btap = Cpad, brow = 9 Cpad); the crop offset (oy, ox) is added to the UPSAMPLED index, after which lin_src (factor 2)
gives two clamped source indices and their weights.

Every case must equal conv3d(crop(up(L))) to 1e-12 relative; every injected fault of the index contract must fail it.
"""
import numpy as np
import pytest
import torch

CPAD = 8   # padded output channels of the buffer (real: 4)


def lin_src(dst, f, n, clamp=True):
    """csrc/wino.hip lin_src in float64; clamp=False drops every clamp (the injected fault)"""
    src = (dst + 0.5) / f - 0.5
    if not clamp:
        i0 = int(np.floor(src))
        return i0, i0 + 1, 1.0 - (src - i0), src - i0
    src = max(src, 0.0)
    i0 = min(int(src), n - 1)
    i1 = min(i0 + 1, n - 1)
    w1 = min(max(src - i0, 0.0), 1.0)
    return i0, i1, 1.0 - w1, w1


def low_sums(L, W, oz, Do, dense):
    """the nine taps' raw sums as the GEMM launch stores them -> (flat buffer, btap, brow)"""
    D, lH, lW, C = L.shape
    Co = W.shape[0]
    rows = Do * lH * lW
    Y = np.zeros((9, Do, lH, lW, Co))
    for kz in range(3):
        Y += np.einsum("zijc,nct->tzijn", L[oz + kz:oz + kz + Do], W[:, :, kz].reshape(Co, C, 9))
    if dense:
        buf = np.zeros((rows, 9, CPAD))
        buf[:, :, :Co] = Y.reshape(9, rows, Co).transpose(1, 0, 2)
        btap, brow = CPAD, 9 * CPAD
    else:
        buf = np.zeros((9, rows, CPAD))
        buf[:, :, :Co] = Y.reshape(9, rows, Co)
        btap, brow = rows * CPAD, CPAD
    # slack behind the buffer: an injected fault may read past its end (or, by a negative index, from its end)
    return np.concatenate([buf.ravel(), np.full(2 * lH * lW * 9 * CPAD, 1e3)]), btap, brow


def out_transform_sum(buf, btap, brow, lH, lW, Co, off, out_shape, fault=None):
    """sum over the taps, raster order, of the bilinear blend of Y_tap at upsampled (oy + y + ky, ox + x + kx)"""
    Do, Ho, Wo = out_shape
    oy, ox = off[1], off[2]
    if fault == "tap_stride":
        btap = btap + lH * lW * brow      # off by one plane
    out = np.zeros((Do, Ho, Wo, Co))
    n = np.arange(Co)
    clamp = fault != "no_clamp"
    for ky in range(3):
        for kx in range(3):
            tap = 3 * kx + ky if fault == "swap" else 3 * ky + kx
            sy, sx = (-ky, -kx) if fault == "negate" else (ky, kx)
            for y in range(Ho):
                if fault == "offset_first":   # the offset applied below the upsampling instead of above it
                    y0, y1, wy0, wy1 = lin_src(y + sy, 2, lH, clamp)
                    y0, y1 = y0 + oy, y1 + oy
                else:
                    y0, y1, wy0, wy1 = lin_src(oy + y + sy, 2, lH, clamp)
                for x in range(Wo):
                    if fault == "offset_first":
                        x0, x1, wx0, wx1 = lin_src(x + sx, 2, lW, clamp)
                        x0, x1 = x0 + ox, x1 + ox
                    else:
                        x0, x1, wx0, wx1 = lin_src(ox + x + sx, 2, lW, clamp)
                    for z in range(Do):
                        def at(i, j):
                            return buf[tap * btap + ((z * lH + i) * lW + j) * brow + n]
                        pa = wx0 * at(y0, x0) + wx1 * at(y0, x1)
                        pb = wx0 * at(y1, x0) + wx1 * at(y1, x1)
                        out[z, y, x] += wy0 * pa + wy1 * pb
    return out


def reference(L, W, off, out_shape):
    """conv3d(crop(up(L))), float64, by torch"""
    Do, Ho, Wo = out_shape
    t = torch.from_numpy(np.ascontiguousarray(L.transpose(3, 0, 1, 2)))[None]
    U = torch.nn.functional.interpolate(t, scale_factor=(1, 2, 2), mode="trilinear", align_corners=False)
    U = U[:, :, off[0]:off[0] + Do + 2, off[1]:off[1] + Ho + 2, off[2]:off[2] + Wo + 2]
    y = torch.nn.functional.conv3d(U, torch.from_numpy(W))
    return y[0].numpy().transpose(1, 2, 3, 0)


# (offset, output extent (y = x), low extent): the low extent is the smallest that covers the stage's input, so the crop starts at
# the map's first row and column (offset 0: the clamped source row -1 is read) and / or ends at its last one (the clamped row lH)
CASES = {
    "off000_38": ((0, 0, 0), 38, 20),   # 2 mod 4; rows 0 .. 39 of 40: both borders
    "off000_36": ((0, 0, 0), 36, 19),   # rows 0 .. 37 of 38: both borders
    "off011_38": ((0, 1, 1), 38, 21),   # odd offset, rows 1 .. 40 of 42: no clamped row
    "off011_36": ((0, 1, 1), 36, 20),   # odd offset, rows 1 .. 38 of 40
    "off011_37": ((0, 1, 1), 37, 20),   # odd offset up to the last row, 39 of 40
}
DO, C, CO = 3, 5, 4
FAULTS = {   # fault -> the cases on which it is no fault at all (and need not fail)
    "swap": (), "negate": (), "tap_stride": (),
    "no_clamp": ("off011_38", "off011_36"),
    "offset_first": ("off000_38", "off000_36"),
}
_CACHE = {}


def _case(name, dense):
    if (name, dense) not in _CACHE:
        off, n, ln = CASES[name]
        rng = np.random.default_rng(sorted(CASES).index(name))
        L = rng.standard_normal((DO + 2 + off[0], ln, ln, C))
        W = rng.standard_normal((CO, C, 3, 3, 3))
        buf, btap, brow = low_sums(L, W, off[0], DO, dense)
        _CACHE[(name, dense)] = (off, (DO, n, n), ln, buf, btap, brow, reference(L, W, off, (DO, n, n)))
    return _CACHE[(name, dense)]


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("dense", [False, True], ids=["batched", "dense"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_identity_with_the_index_contract(name, dense):
    off, shape, ln, buf, btap, brow, ref = _case(name, dense)
    got = out_transform_sum(buf, btap, brow, ln, ln, CO, off, shape)
    assert got.shape == ref.shape
    assert _rel(got, ref) <= 1e-12, _rel(got, ref)


@pytest.mark.parametrize("fault", sorted(FAULTS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_injected_faults_fail(name, fault):
    if name in FAULTS[fault]:
        off, shape, ln, buf, btap, brow, ref = _case(name, False)
        # not a fault on this case: it must still give the reference (the fault list above is not padded with free passes)
        assert _rel(out_transform_sum(buf, btap, brow, ln, ln, CO, off, shape, fault=fault), ref) <= 1e-12
        return
    off, shape, ln, buf, btap, brow, ref = _case(name, False)
    got = out_transform_sum(buf, btap, brow, ln, ln, CO, off, shape, fault=fault)
    assert _rel(got, ref) > 1e-6, (fault, _rel(got, ref))
