"""The wz form of a Winograd stage, F(4x4, 3x3) in (y, x) (x) F(2, 3) along z (csrc/wino.hip; tests/wino_z_ref.py), without a GPU:

  identity   the float64 restatement with the kernels' index contract (pair index, which planes each position combines, the
             clamped overhanging pair, e-major batches) against torch's float64 conv3d, to 1e-12 of the largest output
  faults     each injected fault breaks it: wrong plane pairing for one position, the sign of A^T_z row 2, the plane clamp one
             plane early, G_z over ky instead of kz, the weights' batches b-major -- and the row clamp one row early
  emulation  the split-bf16 arithmetic of the form stays within a small multiple of the plain F(4x4) form's error
  weights    the host-packed images of a 20 -> 24 channel layer (bsmi_debug_wino_pack_host) against the formula, bit for bit
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import layer_ref as L          # noqa: E402
import wino_z_ref as Z         # noqa: E402

# (input D, H, W), Cin, Cout: even Do with whole tiles; odd Do with overhanging tiles (Do = 7, 10 x 10 outputs); one pair only
SHAPES = [((8, 10, 10), 5, 4), ((9, 12, 12), 6, 3), ((3, 7, 9), 3, 2), ((4, 6, 6), 2, 2)]


def _case(shape, cin, cout, seed=0):
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal(shape + (cin,)), -0.25).astype(np.float32)     # post-ReLU-like, not centred
    w = (rng.standard_normal((cout, cin, 3, 3, 3)) / np.sqrt(27 * cin)).astype(np.float32)
    return x, w


def _conv_f64(x, w):
    t = torch.from_numpy(np.ascontiguousarray(x.astype(np.float64).transpose(3, 0, 1, 2)))[None]
    with torch.no_grad():
        y = torch.nn.functional.conv3d(t, torch.from_numpy(w.astype(np.float64)))
    return y[0].numpy().transpose(1, 2, 3, 0)


@pytest.fixture(scope="module")
def refs():
    return {s: (_case(*s), _conv_f64(*_case(*s))) for s in SHAPES}


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "x".join(map(str, c[0])))
def test_identity_in_float64(refs, case):
    (x, w), ref = refs[case]
    got = Z.wino_z_emulate(x, w, exact=True)
    assert got.shape == ref.shape
    rel = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{case}: largest error / largest output {rel:.3e}")
    assert rel <= 1e-12


@pytest.mark.parametrize("fault", Z.FAULTS + ("clamp_rows",))
@pytest.mark.parametrize("case", SHAPES[:2], ids=lambda c: "x".join(map(str, c[0])))
def test_injected_faults_break_the_identity(refs, case, fault):
    (x, w), ref = refs[case]
    if fault == "clamp_rows":
        got = Z.wino_z_emulate(x, w, clamp_rows=1, exact=True)
    else:
        got = Z.wino_z_emulate(x, w, fault=fault, exact=True)
    rel = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{case} {fault}: largest error / largest output {rel:.3e}")
    assert rel > 1e-3, (fault, rel)


def test_plane_contract_by_hand():
    """the contract spelled out with loops on one column of voxels: which planes a position reads, the clamp, the output order"""
    rng = np.random.default_rng(3)
    D = 9                                                  # Do = 7: the last pair overhangs
    x = rng.standard_normal(D)
    g = rng.standard_normal(3)
    Gz = L.WINO[2]["G"]
    Do, R = D - 2, 4
    out = np.zeros(2 * R)
    for r in range(R):
        t = []
        for e in range(4):
            za, zb = min(2 * r + Z.PLANE_A[e], D - 1), min(2 * r + Z.PLANE_B[e], D - 1)
            t.append((x[za] + Z.SIGN_B[e] * x[zb]) * (Gz[e] @ g))
        out[2 * r] = (t[0] + t[1]) + t[2]
        out[2 * r + 1] = (t[1] - t[2]) - t[3]
    ref = np.array([x[z:z + 3] @ g for z in range(Do)])
    assert np.allclose(out[:Do], ref, rtol=0, atol=1e-13)
    assert (Z.PLANE_A, Z.PLANE_B, Z.SIGN_B) == ((0, 1, 2, 1), (2, 2, 1, 3), (-1.0, 1.0, -1.0, -1.0))


def test_split_arithmetic_stays_near_the_plain_form():
    """e_fmt of the wz emulation against that of layer_ref.wino_emulate(.., 4) on the same layer: the extra transform along z
    costs a small factor, not an order of magnitude (1.3 x on the layers measured there)"""
    x, w = _case((9, 14, 14), 40, 24, seed=1)
    ref = _conv_f64(x, w)
    e_wz = np.abs(Z.wino_z_emulate(x, w) - ref).max() / np.abs(ref).max()
    e_w4 = np.abs(L.wino_emulate(x, w, 4) - ref).max() / np.abs(ref).max()
    print(f"largest error / largest output: F(4x4) {e_w4:.3e}, wz {e_wz:.3e}")
    assert e_wz < 1e-4 and e_wz <= 4 * e_w4


def _formula_u(w):
    """U[e][xi][nu][c][n] in double, operation for operation as csrc/wino.hip wino_pack_weights states it (its constants, its
    order of additions), rounded to f32 once"""
    a, b = 0.70710678118654752440, 1.41421356237309504880
    G = np.array([[1, 0, 0], [2. / 3, 2. / 3 * a, 1. / 3], [2. / 3, -2. / 3 * a, 1. / 3], [1. / 12, b / 12, 1. / 6], [1. / 12, -b / 12, 1. / 6],
                  [0, 0, 1]], dtype=np.float64)
    Gz = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)
    g = w.astype(np.float64).transpose(2, 3, 4, 1, 0)                      # (kz, ky, kx, C, N)
    u = np.zeros((3, 6, 6) + g.shape[3:])
    for kz in range(3):
        t = np.stack([np.stack([G[xi, 0] * g[kz, 0, kx] + G[xi, 1] * g[kz, 1, kx] + G[xi, 2] * g[kz, 2, kx] for kx in range(3)]) for xi in range(6)])
        for xi in range(6):
            for nu in range(6):
                u[kz, xi, nu] = t[xi, 0] * G[nu, 0] + t[xi, 1] * G[nu, 1] + t[xi, 2] * G[nu, 2]
    return np.stack([Gz[e, 0] * u[0] + Gz[e, 1] * u[1] + Gz[e, 2] * u[2] for e in range(4)]).astype(np.float32)


def test_host_packed_weights_against_the_formula():
    from bootstrapper_amd import _lib
    lib = _lib.lib
    cin, cout = 20, 24
    w = (np.random.default_rng(7).standard_normal((cout, cin, 3, 3, 3)) / 8).astype(np.float32)
    ie, be, npad, ks = C.c_uint64(), C.c_uint64(), C.c_int(), C.c_int()
    wp = w.ctypes.data_as(C.c_void_p)
    _lib.check(lib.bsmi_debug_wino_pack_host(wp, cout, cin, 1, None, 0, C.byref(ie), C.byref(be), C.byref(npad), C.byref(ks)))
    img = np.zeros(2 * ie.value, dtype=np.uint16)
    _lib.check(lib.bsmi_debug_wino_pack_host(wp, cout, cin, 1, img.ctypes.data_as(C.c_void_p), img.size, None, None, None, None))
    # K = channels only: Cv = 32 is one K-step, padded to an even count
    assert ks.value == 2 and npad.value >= cout and be.value == ks.value * npad.value * 32
    assert ie.value >= 144 * be.value
    U = _formula_u(w)                                         # (4, 6, 6, C, N) f32
    assert np.allclose(U, Z.wino_z_weights(w), rtol=1e-6, atol=1e-9)   # ... and the emulation's weights are the same matrices
    hi = L.bf16_rne(U)
    lo = L.bf16_rne(U - hi)
    want = np.zeros((2, 144, ks.value, npad.value, 32), dtype=np.float32)
    want[0, :, 0, :cout, :cin] = hi.reshape(144, cin, cout).transpose(0, 2, 1)
    want[1, :, 0, :cout, :cin] = lo.reshape(144, cin, cout).transpose(0, 2, 1)
    got = np.stack([img[:144 * be.value], img[ie.value:ie.value + 144 * be.value]]).reshape(want.shape)
    got_f = (got.astype(np.uint32) << 16).view(np.float32)
    assert np.array_equal(got_f.view(np.uint32), want.view(np.uint32))
    assert not img[144 * be.value:ie.value].any()             # the slack rows
    # the plain form from the same entry point: 36 batches, the three z taps inside the chunk
    _lib.check(lib.bsmi_debug_wino_pack_host(wp, cout, cin, 0, None, 0, C.byref(ie), C.byref(be), C.byref(npad), C.byref(ks)))
    assert ks.value == 4 and ie.value >= 36 * be.value
