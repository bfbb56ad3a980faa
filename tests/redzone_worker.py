"""Worker of tests/test_redzones_gpu.py: `redzone_worker.py <family>[,<family>...] <report.json>` runs families of
tests/redzone_cases.py (`all`: every one), one after the other, in a fresh process in which EVERY torch tensor is allocated at its
exact size between two BSMI_GUARD_MB zones of 0xFF (bsmi_debug_torch_malloc / _free of csrc/dev_guard.hip, installed as torch's
allocator before anything touches the device).

In this order: the checker's self-test; a read control (the bytes on both sides of three fresh tensors are 0xFF, so the zones are
where the kernels' stray reads would land and no rounding hides the far one); then per family its parity tests in-process and the
check that no zone is damaged, neither of the live allocations nor of those released meanwhile, so that damage names its family.
The families share a process because a process costs more than most families' tests (torch and the device start in 3 to 4 s); the
GPU suite itself runs in one process.  The report lists per family the entry points of libbsmi.so that were called, and the time.

pytest runs with -s: the guard lines are written by the library to file descriptor 2, and pytest's capture would drop them with the
output of every passing test -- a test whose kernel writes one element too far still passes."""
import ctypes as C
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

families, report_path = sys.argv[1], sys.argv[2]
assert os.environ.get("BSMI_GUARD_MB"), "BSMI_GUARD_MB must be set"

import torch  # noqa: E402
from torch.cuda.memory import CUDAPluggableAllocator, change_current_allocator  # noqa: E402

lib_path = os.environ.get("BSMI_LIB") or os.path.join(ROOT, "bootstrapper_amd", "libbsmi.so")
change_current_allocator(CUDAPluggableAllocator(lib_path, "bsmi_debug_torch_malloc", "bsmi_debug_torch_free"))

import pytest  # noqa: E402
import redzone_cases  # noqa: E402
from bootstrapper_amd import _lib  # noqa: E402

# count the entry points that are called: the wrappers of the package look them up on the CDLL object at call time
called = set()


def _counting(name, fn):
    def call(*args):
        called.add(name)
        return fn(*args)
    return call


check_guards = _lib.lib.bsmi_debug_check_guards
for name in _lib.SYMBOLS:
    if name.startswith("bsmi_"):
        setattr(_lib.lib, name, _counting(name, getattr(_lib.lib, name)))

rc = _lib.lib.bsmi_debug_guard_selftest()
assert rc == 0, f"bsmi_debug_guard_selftest() = {rc}: the checker does not see bytes written into its zones"
print("self-test ok", flush=True)

# read control: one element before and one behind each tensor, read with the runtime that the process has bound.  torch loads its
# copy of it privately (dlopen(NULL) does not see hipMemcpy) and under a path of its own, and a second copy must not be loaded
# (bootstrapper_amd/_lib.py), so the loaded one is taken from the process's own map
hip_path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
hip = C.CDLL(hip_path)
hip.hipMemcpy.restype = C.c_int
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
for dtype in (torch.int64, torch.float32, torch.uint8):
    t = torch.zeros(1000, dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    e = t.element_size()
    for where, addr in (("before", t.data_ptr() - e), ("behind", t.data_ptr() + 1000 * e)):
        buf = (C.c_ubyte * e)()
        assert hip.hipMemcpy(buf, addr, e, 2) == 0   # hipMemcpyDeviceToHost
        assert bytes(buf) == b"\xff" * e, f"the element {where} a tensor of 1000 {dtype} reads {bytes(buf).hex()}, not 0xFF bytes"
    del t
print("read control ok", flush=True)

os.chdir(ROOT)
families = list(redzone_cases.FAMILIES) if families == "all" else families.split(",")
report = {}
for family in families:
    called.clear()
    t0 = time.time()
    status = pytest.main(list(redzone_cases.FAMILIES[family]) + ["-m", "gpu", "-q", "-x", "-s", "-p", "no:cacheprovider"])
    assert int(status) == 0, f"{family}: pytest exit status {int(status)}"
    torch.cuda.synchronize()
    bad = check_guards()
    assert bad == 0, f"{family}: {bad} guard zones written to (see the `guard:` lines above)"
    gc.collect()
    torch.cuda.synchronize()
    bad = check_guards()
    assert bad == 0, f"{family}: {bad} guard zones written to, found after the last tensors were released"
    report[family] = {"called": sorted(called), "seconds": round(time.time() - t0, 2)}
    with open(report_path, "w") as f:      # after every family: the report says how far the run came
        json.dump(report, f)
    print(f"{family}: {len(called)} entry points called, {report[family]['seconds']:.1f} s, guards intact", flush=True)
print("guards intact", flush=True)
