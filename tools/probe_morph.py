"""Dev tool: `bs refine morph` on one GPU -> JSON lines.

device  the device calls alone on a synthetic, device-resident 512 x 1024 x 1024 u64 label volume (jittered cells with
        background gaps between them and background specks inside), timed with events after a warm-up, median of 5: dilate and
        erode at 1 and 4 iterations, in 3-D and per section (bsmi_label_morph_u64), and fill_holes once
        (bsmi_label_fill_holes_u64, its host decision included).  GB/s at the algorithmic 16 bytes per voxel and iteration and
        the fraction of 6.3 TB/s.
e2e     one `bs refine morph` (closing, 2 iterations, default context and block size) on an on-disk store of 64 x 512 x 512,
        wall clock, next to the device share: the same blocks' operations alone, timed with events.
`--only device` / `--only e2e`: one part, e.g. the device part under `rocprofv3 --kernel-trace --stats --`."""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from bootstrapper_amd import _lib
from bootstrapper_amd.post.engine import label_fill_holes, label_morph
from bootstrapper_amd.refine import apply_morph, morph, morph_blocks

dev = torch.device("cuda", 0)
HBM = 6.3e12


def cells_with_gaps(shape, cell, seed, gap=2, specks=1e-4):
    """u64 ids of jittered cells, made on the device: `gap` background voxels between neighbouring cells on every axis and
    background specks (holes) inside them"""
    g = torch.Generator(device=dev).manual_seed(seed)
    D, H, W = shape
    z = torch.arange(D, device=dev).view(-1, 1, 1)
    y = torch.arange(H, device=dev).view(1, -1, 1) + torch.randint(0, cell[1] // 2, (D, 1, W), device=dev, generator=g)
    x = torch.arange(W, device=dev).view(1, 1, -1) + torch.randint(0, cell[2] // 2, (D, H, 1), device=dev, generator=g)
    ids = (z // cell[0]) * 1_000_003 + (y // cell[1]) * 1009 + x // cell[2] + (1 << 40)
    ids = ids * ((z % cell[0] >= gap) & (y % cell[1] >= gap) & (x % cell[2] >= gap))
    return (ids * (torch.rand(shape, device=dev, generator=g) >= specks)).contiguous()


def events(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def device_part(shape=(512, 1024, 1024)):
    nv = int(np.prod(shape))
    lab = cells_with_gaps(shape, (16, 96, 96), 1)
    out, tmp = torch.empty_like(lab), torch.empty_like(lab)
    res = {"background_fraction": float((lab == 0).float().mean())}
    for op, code in (("dilate", _lib.MORPH_DILATE), ("erode", _lib.MORPH_ERODE)):
        for xy in (False, True):
            for n in (1, 4):
                ms = events(lambda: label_morph(lab, code, n, xy, out=out, tmp=tmp))
                res[f"{op}_{'xy' if xy else '3d'}_n{n}"] = {"ms": ms, "GBps": 16 * nv * n / ms / 1e6, "hbm_fraction": 16 * nv * n / ms / 1e-3 / HBM}
    filled = []
    ms = events(lambda: filled.append(label_fill_holes(lab, False, out=out)[1]))
    res["fill_holes_3d"] = {"ms": ms, "components_filled": filled[-1], "ms_per_1e8_voxels": ms * 1e8 / nv}
    return {"part": "device", "shape": list(shape), "voxels": nv, "bytes_per_voxel_per_iteration": 16, **res}


def e2e_part(shape=(64, 512, 512), chunks=(32, 128, 128), op="closing", iterations=2):
    from bootstrapper_amd.zarr_io import open_ds, prepare_ds
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR")) as tmp:
        store = os.path.join(tmp, "vol.zarr")
        vol = cells_with_gaps(shape, (16, 64, 64), 9).cpu().numpy().view(np.uint64)
        d = prepare_ds(f"{store}/seg", shape, offset=(0, 0, 0), voxel_size=(40, 4, 4), chunk_shape=chunks, dtype=np.uint64,
                       axis_names=["z", "y", "x"], units=["nm"] * 3)
        d[:] = vol
        walls = []
        for _ in range(3):   # the first run also loads code objects and fills the allocator's and the writer's pools
            torch.cuda.synchronize()
            t = time.perf_counter()
            morph(f"{store}/seg", f"{store}/out", op=op, iterations=iterations)
            walls.append(time.perf_counter() - t)
        device_ms = 0.0
        for _, read in morph_blocks(shape, chunks, 2048, 64, False):
            block = torch.from_numpy(vol[tuple(slice(lo, hi) for lo, hi in read)].view(np.int64).copy()).to(dev)
            device_ms += events(lambda: apply_morph(block.clone(), op, iterations, False))
        return {"part": "e2e", "shape": list(shape), "chunks": list(chunks), "op": op, "iterations": iterations,
                "bs_refine_morph_s": walls, "device_ms_all_blocks": device_ms, "output_bytes": int(open_ds(f"{store}/out")[:].nbytes)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["device", "e2e"])
    a = ap.parse_args()
    if a.only in (None, "device"):
        print(json.dumps(device_part()), flush=True)
        torch.cuda.empty_cache()
    if a.only in (None, "e2e"):
        print(json.dumps(e2e_part()), flush=True)


if __name__ == "__main__":
    main()
