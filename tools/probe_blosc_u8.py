"""Dev tool: device-event medians of the two launches of `bsmi_blosc_encode_dev_u8` (csrc/blosc_dev_u8.hip) for one chunk
(6, 128, 128, 128) of affinity-like data (the recipe of tests/blosc_u8_ref.py's fixture B) and of uniform noise, in ms and GB/s
of chunk bytes.  python tools/probe_blosc_u8.py [repetitions]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from bootstrapper_amd import _lib

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
shape = (6, 128, 128, 128)
dev = torch.device("cuda", 0)
print(torch.cuda.get_device_name(0), flush=True)


def affinity_like(seed):
    """|smooth field| through a steep sigmoid + noise, on the device: saturates inside objects, drops at boundaries"""
    g = torch.Generator(device=dev).manual_seed(seed)
    f = torch.randn((1, 1) + shape[1:], device=dev, generator=g)
    k = torch.exp(-0.5 * (torch.arange(-12, 13, device=dev, dtype=torch.float32) / 4.0) ** 2)
    k = k / k.sum()
    for axis in (3, 4):   # separable Gaussian, sigma 4 along y and x (sigma 1 along z is left out: it changes little)
        view = [1, 1, 1, 1, 1]
        view[axis] = 25
        pad = [0, 0, 0, 0, 0, 0]
        pad[2 * (4 - axis)] = pad[2 * (4 - axis) + 1] = 12
        f = torch.nn.functional.conv3d(torch.nn.functional.pad(f, pad, mode="circular"), k.view(view))
    f = f[0, 0] / f.std()
    x = 40 * (f.abs() - 0.3)[None] + 2.0 * torch.randn(shape, device=dev, generator=g)
    return torch.floor(255.0 / (1.0 + torch.exp(-x))).to(torch.uint8)


def measure(name, src):
    cb = src.numel()
    slot = int(_lib.lib.bsmi_blosc_dev_u8_frame_bound(cb))
    ns = int(_lib.lib.bsmi_blosc_dev_u8_scratch_bytes(1, cb))
    scratch, frames = torch.empty(ns, dtype=torch.uint8, device=dev), torch.empty(slot, dtype=torch.uint8, device=dev)
    sizes = torch.zeros(1, dtype=torch.int32, device=dev)
    arr = lambda v: (C.c_int64 * len(v))(*v)
    st = torch.cuda.current_stream()
    times = []
    for _ in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        _lib.check(_lib.lib.bsmi_blosc_encode_dev_u8(0, C.c_void_p(src.data_ptr()), arr(src.stride()[:3]), 1, arr([0, 0, 0, 0]), arr(shape), arr(shape),
                                                      C.c_void_p(scratch.data_ptr()), ns, C.c_void_p(frames.data_ptr()), slot, C.c_void_p(sizes.data_ptr()),
                                                      C.c_void_p(st.cuda_stream)))
        b.record(st)
        b.synchronize()
        times.append(a.elapsed_time(b))
    ms = float(np.median(times[3:]))
    size = int(sizes.item())
    print(f"{name}: chunk {cb} bytes -> frame {size} bytes ({size / cb:.3f}); both launches {ms:.3f} ms median of {reps} "
          f"(min {min(times[3:]):.3f}, max {max(times[3:]):.3f}) = {cb / ms / 1e6:.1f} GB/s", flush=True)


measure("affinity-like", affinity_like(2))
measure("noise", torch.randint(0, 256, shape, dtype=torch.uint8, device=dev))
measure("zeros", torch.zeros(shape, dtype=torch.uint8, device=dev))
