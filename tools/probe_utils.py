"""Dev tool: the raw-mask closing (csrc/utils.hip, disk(10)) on sections of the size a user runs, timed with device events, no
profiler, next to the reference's own operation on the CPU (tests/utils_ref.closing = skimage binary_closing, one thread) on the
same sections.  The CPU side may be limited to the first `cpu_sections` sections; its time is then scaled to all of them and the
line says so.
usage: probe_utils.py [sections] [edge] [reps] [cpu_sections]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np, torch
import utils_ref as R
from bootstrapper_amd.utils import MASK_RADIUS, closing_work_bytes, mask_closing

sections = int(sys.argv[1]) if len(sys.argv) > 1 else 125
edge = int(sys.argv[2]) if len(sys.argv) > 2 else 1250
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
cpu_sections = int(sys.argv[4]) if len(sys.argv) > 4 else sections
dev = torch.device("cuda", 0)
rng = np.random.default_rng(0)
shape = (sections, edge, edge)
# sparse texture with empty margins, as raw data with a blank border has: the closing fills the inside
raw = ((rng.random(shape) < 0.01) * rng.integers(1, 256, shape)).astype(np.uint8)
raw[:, : edge // 10] = 0
raw[:, :, -edge // 8:] = 0
src = torch.from_numpy(raw).to(dev)
out = torch.empty_like(src)
work = torch.empty((closing_work_bytes(shape, MASK_RADIUS) + 7) // 8, dtype=torch.int64, device=dev)
for _ in range(3):
    mask_closing(src, MASK_RADIUS, out, work)
torch.cuda.synchronize()
times = []
for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    mask_closing(src, MASK_RADIUS, out, work)
    e1.record()
    e1.synchronize()
    times.append(e0.elapsed_time(e1))
times.sort()
got = out.cpu().numpy()
fp = R.disk(MASK_RADIUS)
t0 = time.perf_counter()
want = np.stack([R.closing(np.pad(s != 0, 2 * MASK_RADIUS), fp)[2 * MASK_RADIUS:-2 * MASK_RADIUS, 2 * MASK_RADIUS:-2 * MASK_RADIUS] for s in raw[:cpu_sections]])
cpu = (time.perf_counter() - t0) * sections / cpu_sections
same = np.array_equal(got[:cpu_sections], want.astype(np.uint8))
gpu = times[len(times) // 2]
nbytes = 2 * raw.size + 2 * work.numel() * 8
print(f"closing disk({MASK_RADIUS}) on {sections} sections of {edge} x {edge}: device median {gpu:.3f} ms (min {times[0]:.3f}, max {times[-1]:.3f}, {reps} reps; "
      f"{nbytes / gpu / 1e6:.0f} GB/s of the {nbytes / 1e6:.0f} MB it must move), CPU {cpu:.1f} s"
      + (f" (scaled from {cpu_sections} sections)" if cpu_sections != sections else "")
      + f", ratio {cpu * 1e3 / gpu:.0f}; result mean {got.mean():.3f}, bit-equal on the CPU's sections: {same}")
sys.exit(0 if same else 1)
