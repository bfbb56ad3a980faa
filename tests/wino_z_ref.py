"""The "wz" form of a Winograd stage (csrc/wino.hip, WinoInArgs::wz): F(4x4, 3x3) in (y, x) (x) F(2, 3) along z, on the CPU.

One function states the form with the kernels' index contract, twice over:

  exact=True    float64 throughout, nothing rounded: the identity itself.  tests/test_wino_z_cpu.py holds it against torch's
                conv3d to 1e-12 and shows that each injected fault breaks it.
  exact=False   the arithmetic of the split mode as tests/layer_ref.py wino_emulate states it for the plain form: the plane
                combination and B^T d B in f32, V and U stored as (hi, lo) bf16 pairs, M = Vhi Uhi + Vlo Uhi + Vhi Ulo accumulated
                in float64, A^T M A in f32 per position, then the two output planes in f32 in the kernel's fixed order.  It is the
                `emu_pre` of layer_ref.allowances for a stage that plan_steps() reports with wino_z.

The contract (include/bsmi.h BSMI_STEP_WINO_Z; csrc/wino.h):
  pair r = z // 2 of output planes, R = ceil(Do / 2) pairs; position e = 0 .. 3 of a pair combines exactly two planes of the
  layer's input, (first, second, sign of the second):
      e = 0: (2r, 2r+2, -)   e = 1: (2r+1, 2r+2, +)   e = 2: (2r+2, 2r+1, -)   e = 3: (2r+1, 2r+3, -)
  (the rows of B^T_z = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]); a plane index past the input (the last pair of an odd Do) is
  clamped to the last plane, as rows and columns of overhanging tiles are; the second plane of that pair is never stored.
  Batches are e-major: batch 36 e + 6 xi + nu, V[batch][r][ty][tx][c] and U[batch][c][n] with
      U[e] = sum_kz G_z[e][kz] (G g_kz G^T),   G_z = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]
  made in double and rounded to f32 once.  Output: t_e = A^T M_e A, out[2r] = (t0 + t1) + t2, out[2r+1] = (t1 - t2) - t3.
"""
import numpy as np

import layer_ref as L

PLANE_A = (0, 1, 2, 1)
PLANE_B = (2, 2, 1, 3)
SIGN_B = (-1.0, 1.0, -1.0, -1.0)
FAULTS = ("pairing", "atz_sign", "clamp_plane", "gz_on_ky", "b_major")


def wino_z_weights(w, exact=False, fault=None):
    """U (4, 6, 6, C, N): float64 when exact, else the f32 values the packing splits."""
    g = np.asarray(w, dtype=np.float32).astype(np.float64)                  # (N, C, kz, ky, kx)
    G, Gz = L.WINO[4]["G"], L.WINO[2]["G"]
    if fault == "gz_on_ky":
        U = np.einsum("ey,az,nczyx,bx->eabcn", Gz, G, g, G, optimize=True)    # the z matrix over ky, the in-plane one over kz
    else:
        U = np.einsum("ez,ay,nczyx,bx->eabcn", Gz, G, g, G, optimize=True)
    return U if exact else U.astype(np.float32)


def wino_z_emulate(x, w, clamp_rows=0, fault=None, exact=False):
    """Sums of a valid 3x3x3 convolution (no bias) in the wz form.  x: (D, H, W, C) values as the device holds them, w: (Cout, C,
    3, 3, 3) float32.  Returns (D - 2, H - 2, W - 2, Cout) float64.
    clamp_rows (fault injection, as layer_ref.wino_emulate): the row clamp sets in that many rows too early.
    fault: one of FAULTS -- "pairing": position 1 takes plane 2r+3 for 2r+2; "atz_sign": the sign of t2 in the second output
    plane; "clamp_plane": the plane clamp sets in one plane too early; "gz_on_ky": G_z over ky instead of kz; "b_major": the
    weights' batches b-major (4 b + e) against an e-major V."""
    assert fault is None or fault in FAULTS, fault
    ft = np.float64 if exact else np.float32
    mats = L.WINO[4]
    m, T = 4, 6
    x = np.asarray(x, dtype=ft)
    D, H, W, C = x.shape
    Do, Ho, Wo = D - 2, H - 2, W - 2
    R = -(-Do // 2)
    Ty, Tx = -(-Ho // m), -(-Wo // m)
    # the plane combinations, element-wise, one rounding in f32
    r2 = 2 * np.arange(R)
    last = D - 1 - (1 if fault == "clamp_plane" else 0)
    dz = []
    for e in range(4):
        pb = 3 if (fault == "pairing" and e == 1) else PLANE_B[e]
        za, zb = np.minimum(r2 + PLANE_A[e], last), np.minimum(r2 + pb, last)
        dz.append((x[za] + ft(SIGN_B[e]) * x[zb]).astype(ft))
    dz = np.stack(dz)                                              # (4, R, H, W, C)
    # the unchanged in-plane transform (layer_ref.wino_emulate)
    yi = np.minimum(np.arange(Ty * m + 2), H - 1 - clamp_rows)
    xi = np.minimum(np.arange(Tx * m + 2), W - 1)
    xp = dz[:, :, yi][:, :, :, xi]
    ty = (np.arange(Ty) * m)[:, None] + np.arange(T)[None]
    tx = (np.arange(Tx) * m)[:, None] + np.arange(T)[None]
    d = xp[:, :, ty][:, :, :, :, tx]                               # (4, R, Ty, T, Tx, T, C)
    BT = mats["BT"].astype(ft)
    V = np.einsum("ai,erpiqjc,bj->eabrpqc", BT, d, BT, optimize=True).astype(ft)
    U = wino_z_weights(w, exact, fault)
    N = U.shape[-1]
    # 144 batches, e-major: batch 36 e + 6 xi + nu
    Vb = V.reshape(4 * T * T, R * Ty * Tx, C)
    if fault == "b_major":
        Ub = np.ascontiguousarray(U.transpose(1, 2, 0, 3, 4)).reshape(4 * T * T, C, N)
    else:
        Ub = U.reshape(4 * T * T, C, N)
    if exact:
        Mx = np.matmul(Vb, Ub)
    else:
        Vh, Vl = L.split_bf16(Vb)
        Uh, Ul = L.split_bf16(Ub)
        Mx = np.matmul(Vh + Vl, Uh) + np.matmul(Vh, Ul)
    Mx = Mx.reshape(4, T, T, R, Ty, Tx, N)
    AT = mats["AT"].astype(ft)
    t = np.einsum("ua,eabrpqn,vb->erpuqvn", AT, Mx.astype(ft), AT, optimize=True).astype(ft)   # (4, R, Ty, m, Tx, m, N)
    o0 = ((t[0] + t[1]).astype(ft) + t[2]).astype(ft)
    if fault == "atz_sign":
        o1 = ((t[1] + t[2]).astype(ft) - t[3]).astype(ft)
    else:
        o1 = ((t[1] - t[2]).astype(ft) - t[3]).astype(ft)
    Y = np.stack([o0, o1], axis=1).reshape(2 * R, Ty * m, Tx * m, N)
    return Y[:Do, :Ho, :Wo].astype(np.float64)
