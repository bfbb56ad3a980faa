"""Does a normalised per-output error separate the split-bf16 format's own error from small kernel faults?
GEMM view of one conv stage: out[m, n] = sum_k x[m, k] w[k, n] + b[n];  K = taps * Cin.

The experiment behind the gates of tests/layer_ref.py (per-launch parity, tests/test_layers_gpu.py).  Two scales per output:
A = sum |x| |w| + |b| and S = sqrt(sum x^2 w^2 + b^2).  Against S the error of a number format is a constant -- the split
format 1.9e-5 ... 2.2e-5 for K from 324 to 48 600, f32 accumulation 1.5e-6 ... 2.0e-6, plain bf16 1.0e-2 ... 1.1e-2 -- and
the smallest fault (the lo part of one tap's weights lost) stays 70 times above the split format; against A everything
shrinks with sqrt(K) and a gate would have to depend on the layer.  Output (seed 0, numpy with a blocked BLAS sum):

K = 324
   split            max err/A 2.362e-06   max err/S 1.878e-05
   split_f32acc     max err/A 2.373e-06   max err/S 1.881e-05
   f32              max err/A 2.180e-07   max err/S 1.889e-06
   fault_a_lo_tap   max err/A 3.142e-04   max err/S 2.386e-03
   fault_d_kstep    max err/A 2.011e-01   max err/S 1.377e+00
   fault_c_bias     max err/A 2.021e-03   max err/S 1.696e-02
   bf16             max err/A 1.186e-03   max err/S 9.543e-03
K = 1620
   split            max err/A 1.134e-06   max err/S 2.028e-05
   split_f32acc     max err/A 1.156e-06   max err/S 2.060e-05
   f32              max err/A 1.116e-07   max err/S 1.978e-06
   fault_a_lo_tap   max err/A 9.624e-05   max err/S 1.664e-03
   fault_d_kstep    max err/A 4.772e-02   max err/S 8.455e-01
   fault_c_bias     max err/A 9.602e-03   max err/S 1.707e-01
   bf16             max err/A 6.063e-04   max err/S 1.086e-02
K = 8100
   split            max err/A 5.478e-07   max err/S 2.138e-05
   split_f32acc     max err/A 5.568e-07   max err/S 2.173e-05
   f32              max err/A 3.826e-08   max err/S 1.517e-06
   fault_a_lo_tap   max err/A 3.816e-05   max err/S 1.526e-03
   fault_d_kstep    max err/A 8.560e-03   max err/S 3.462e-01
   fault_c_bias     max err/A 1.548e-03   max err/S 6.302e-02
   bf16             max err/A 2.600e-04   max err/S 1.044e-02
K = 48600
   split            max err/A 1.928e-07   max err/S 1.916e-05
   split_f32acc     max err/A 1.909e-07   max err/S 1.897e-05
   f32              max err/A 1.995e-08   max err/S 1.976e-06
   fault_a_lo_tap   max err/A 1.374e-05   max err/S 1.364e-03
   fault_d_kstep    max err/A 1.241e-03   max err/S 1.236e-01
   fault_c_bias     max err/A 9.640e-04   max err/S 9.545e-02
   bf16             max err/A 1.148e-04   max err/S 1.141e-02
K = 2700
   split            max err/A 7.897e-07   max err/S 1.897e-05
   split_f32acc     max err/A 7.894e-07   max err/S 1.889e-05
   f32              max err/A 7.033e-08   max err/S 1.697e-06
   fault_a_lo_tap   max err/A 1.141e-04   max err/S 2.617e-03
   fault_d_kstep    max err/A 2.490e-02   max err/S 5.884e-01
   fault_c_bias     max err/A 8.514e-03   max err/S 2.046e-01
   bf16             max err/A 4.347e-04   max err/S 1.038e-02
"""
import numpy as np

rng = np.random.default_rng(0)


def bf16(a):
    a = np.asarray(a, np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000          # round to nearest even
    return u.astype(np.uint32).view(np.float32)


def split(a):
    hi = bf16(a)
    lo = bf16(np.asarray(a, np.float32) - hi)
    return hi.astype(np.float64), lo.astype(np.float64)


def run(taps, cin, cout, M=2048):
    K = taps * cin
    x = np.maximum(rng.standard_normal((M, K)), 0).astype(np.float32)       # post-ReLU activations
    w = (rng.standard_normal((K, cout)) * (1.5 / np.sqrt(K))).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    ref = x64 @ w64 + b
    A = np.abs(x64) @ np.abs(w64) + np.abs(b)
    S = np.sqrt((x64 ** 2) @ (w64 ** 2) + b.astype(np.float64) ** 2)
    xh, xl = split(x)
    wh, wl = split(w)
    good = xh @ wh + xl @ wh + xh @ wl + b                                     # the split mode, exact accumulation
    good32 = (xh.astype(np.float32) @ wh.astype(np.float32) + xl.astype(np.float32) @ wh.astype(np.float32)
              + xh.astype(np.float32) @ wl.astype(np.float32) + b).astype(np.float64)   # ... f32 accumulation (BLAS order)
    f32 = (x @ w + b).astype(np.float64)
    # faults
    wl_a = wl.copy(); wl_a[:cin] = 0                                           # (a) one tap's weights lose their lo part
    fa = xh @ wh + xl @ wh + xh @ wl_a + b
    xs = x64.copy(); xs[:, :32] = 0                                            # (d) one K-step of 32 channels of one tap dropped
    fd = xs @ w64 + b
    fb = ref.copy(); fb[:, 0] -= b[0]                                          # (c) bias of one channel omitted
    bf = bf16(x).astype(np.float64) @ bf16(w).astype(np.float64) + b           # plain bf16 operands
    out = {}
    for name, got in (("split", good), ("split_f32acc", good32), ("f32", f32), ("fault_a_lo_tap", fa), ("fault_d_kstep", fd),
                      ("fault_c_bias", fb), ("bf16", bf)):
        d = np.abs(got - ref)
        out[name] = (float((d / A).max()), float((d / S).max()))
    return K, out


for taps, cin, cout in ((27, 12, 12), (27, 60, 60), (27, 300, 64), (27, 1800, 32), (9, 300, 64)):
    K, o = run(taps, cin, cout)
    print(f"K = {K}")
    for k, (ea, es) in o.items():
        print(f"   {k:16s} max err/A {ea:.3e}   max err/S {es:.3e}")
