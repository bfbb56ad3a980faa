"""Dev tool: the non-blockwise watershed on full-size sections on one GPU, timed with device events -> one JSON line.
Fragments (seeds + wide flood) of CREMI-shaped sections, (4, 1250, 1250) and (125, 1250, 1250), the "half" (one straight
edge) and white-noise slices, mean agglomeration of (4, 1250, 1250), and the device memory of a (125, 1250, 1250) handle.
fragments_ms: the fragments call, every slice side by side (one workgroup each) -- i.e. the ms per slice of the slowest one;
us_per_pop: that time over the largest number of voxels one slice floods (each is popped once).
`--only half`: that case alone, e.g. under `rocprofv3 --kernel-trace --stats --` for the seeds kernel's share.
`--stats`: per case, where the wide flood's pops go (heap moves in LDS and in spilled levels, window fetches, spilled reads of
a push) and the pop loop's own time per pop, from in-kernel counters of a -DBSMI_FLOOD_STATS build passed as BSMI_LIB:
  make -C bootstrapper_amd/csrc CXXFLAGS_EXTRA=-DBSMI_FLOOD_STATS OUT=../libbsmi_flood_stats.so BUILD=build_flood_stats
  BSMI_LIB=$PWD/bootstrapper_amd/libbsmi_flood_stats.so python tools/probe_large_sections.py --stats
(the times of such a run include the counters; take them from a run of the product library)"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy.ndimage import gaussian_filter
from bootstrapper_amd import _lib
from bootstrapper_amd.post.engine import SegEngine

dev = torch.device("cuda", 0)


def blobby(shape, seed):
    a = gaussian_filter(np.random.default_rng(seed).random((3,) + shape, dtype=np.float32), sigma=(0, 0, 6, 6))
    return ((a - a.min()) / (a.max() - a.min()) * 255).astype(np.uint8)


def timed(fn, reps=2):
    best = None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return best, out


STATS = None   # (C buffer of the 16 counters) when --stats
STAT_NAMES = ["pops", "lds_moves", "window_fetches", "spill_moves", "pushes", "push_moves", "push_spill_reads", "last_spill_reads",
              "max_heap", "loop_ticks", "slices"]


def read_stats(reset):
    if STATS is not None and _lib.lib.bsmi_debug_flood_stats(STATS, 1 if reset else 0) != 0:
        raise RuntimeError("bsmi_debug_flood_stats failed")
    return [int(v) for v in STATS] if STATS is not None else None


def fragments(name, affs, msd=10, reps=2):
    t = torch.from_numpy(affs).to(dev)
    read_stats(True)
    free0 = torch.cuda.mem_get_info(0)[0]
    eng = SegEngine(affs.shape[1:], 0)
    torch.cuda.synchronize()
    handle_mb = (free0 - torch.cuda.mem_get_info(0)[0]) / 2**20
    ms, (frags, mx) = timed(lambda: eng.ws_fragments(t, True, msd), reps)
    pops = int((frags != 0).flatten(1).sum(1).max().item())
    r = {"case": name, "shape": list(affs.shape[1:]), "fragments_ms": round(ms, 2), "max_id": int(mx.item()),
         "pops_max_slice": pops, "us_per_pop": round(ms * 1000 / max(pops, 1), 3), "handle_mb": round(handle_mb, 1)}
    st = read_stats(True)
    if st is not None:   # per pop, over every slice of every rep
        c = dict(zip(STAT_NAMES, st))
        p = max(c["pops"], 1)
        r["flood_stats"] = {k: round(c[k] / p, 3) for k in STAT_NAMES[1:8]}
        r["flood_stats"].update(max_heap=c["max_heap"], loop_us_per_pop=round(c["loop_ticks"] / 100.0 / p, 3))
    return r, eng, t, frags


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="one case: cremi4 | cremi125 | half | noise")
    ap.add_argument("--stats", action="store_true", help="in-kernel counters of the wide flood (a -DBSMI_FLOOD_STATS build as BSMI_LIB)")
    args = ap.parse_args()
    global STATS
    if args.stats:
        if not hasattr(_lib.lib, "bsmi_debug_flood_stats"):
            raise SystemExit("--stats needs a -DBSMI_FLOOD_STATS build of the library passed as BSMI_LIB")
        _lib.lib.bsmi_debug_flood_stats.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
        STATS = (C.c_ulonglong * 16)()
    cases, out = ["cremi4", "cremi125", "half", "noise"], []
    for c in cases if args.only is None else [args.only]:
        if c == "cremi4":
            r, eng, t, frags = fragments(c, blobby((4, 1250, 1250), 0))
            ms, segs = timed(lambda: eng.agglomerate_mean(t, frags, [0.2, 0.35, 0.5]))
            eng.status()
            r["agglomerate_mean_ms"] = round(ms, 2)
        elif c == "cremi125":   # 4 distinct sections repeated: every slice has a CREMI section's work
            a4 = blobby((4, 1250, 1250), 1)
            r = fragments(c, np.ascontiguousarray(np.tile(a4, (1, 32, 1, 1))[:, :125]), reps=1)[0]
        elif c == "half":
            a = np.zeros((3, 1, 1250, 1250), np.uint8)
            a[:, :, :, :625] = 255
            r = fragments(c, a)[0]
        else:
            r = fragments(c, np.random.default_rng(2).integers(0, 256, (3, 1, 1024, 1200), dtype=np.uint8), msd=2)[0]
        out.append(r)
        torch.cuda.empty_cache()
    print(json.dumps({"large_sections": out}))


if __name__ == "__main__":
    main()
