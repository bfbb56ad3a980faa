"""Dev tool: `bs evaluate` on one GPU -> JSON lines.

device  the two device passes on a synthetic, device-resident 512 x 1024 x 1024 volume (Voronoi-like u64 ids, 6-channel u8
        affinities, a u8 mask), timed with events after a warm-up: the affinity-error pass (bsmi_eval_aff_errors_u8, the whole
        volume as one tile of 128^3 chunks, the block of `bs predict` in bench.py) and the contingency pass (bsmi_eval_pairs_u64 +
        read-out).  Algorithmic bytes per voxel, GB/s and the fraction of 6.3 TB/s.
e2e     `bs evaluate` (run_evaluation, both modes) on an on-disk store with four segmentations, wall clock, next to
        tests/eval_ref.py on the same data (one CPU process per segmentation) and a check that the outputs agree.
lsd     the LSD-error pass (bsmi_eval_lsd_errors_u8) on device-resident volumes at chunks (8, 256, 256) and 128^3 with the
        reference's margin (2, 50, 50), voxel size (40, 8, 8), sigma 80, downsample 2: ms per 1e8 ROI voxels; next to it
        bsmi_train_lsd_targets (the per-voxel brute force) on one chunk's grown label array, scaled to the same voxels; and
        `bs evaluate --pred` with the opt-in on the e2e store with a 3d_lsds dataset.  The split into stages comes from running
        this part under `rocprofv3 --kernel-trace --stats --` (kernels lsd_sub / lsd_desc / lsd_norm / lsd_xy / lsd_zclose).
`--only device` / `--only e2e` / `--only lsd`: one part, e.g. the device part under `rocprofv3 --kernel-trace --stats --`."""
import argparse, ctypes as C, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from bootstrapper_amd import _lib
from bootstrapper_amd.evaluate import EvalDevice

dev = torch.device("cuda", 0)
HBM = 6.3e12
NHOOD = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0], [0, 8, 0], [0, 0, 8]]


def voronoi_like(shape, cell, seed, halo=(0, 0, 0), jitter=True):
    """u64 ids of jittered cells, made on the device; `halo` extra zero voxels after the volume on every axis.  The jitter is
    drawn per row, so object boundaries are ragged over a quarter of a cell; jitter = False gives plain boxes"""
    g = torch.Generator(device=dev).manual_seed(seed)
    D, H, W = shape
    z = torch.arange(D, device=dev).view(-1, 1, 1)
    y = torch.arange(H, device=dev).view(1, -1, 1)
    x = torch.arange(W, device=dev).view(1, 1, -1)
    jy = torch.randint(0, cell[1] // 2, (D, 1, W), device=dev, generator=g)
    jx = torch.randint(0, cell[2] // 2, (D, H, 1), device=dev, generator=g)
    if not jitter:
        jy, jx = jy * 0, jx * 0
    ids = (z // cell[0]) * 1_000_003 + ((y + jy) // cell[1]) * 1009 + (x + jx) // cell[2] + (1 << 40)
    out = torch.zeros((D + halo[0], H + halo[1], W + halo[2]), dtype=torch.int64, device=dev)
    out[:D, :H, :W] = ids
    return out


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


def device_part(shape=(512, 1024, 1024), chunk=(128, 128, 128)):
    nv = int(np.prod(shape))
    eng = EvalDevice(0)
    halo = tuple(max(o[d] for o in NHOOD) for d in range(3))
    seg = voronoi_like(shape, (16, 96, 96), 1, halo)
    pred = torch.randint(0, 256, (6,) + shape, dtype=torch.uint8, device=dev)
    mask = (torch.rand(shape, device=dev) < 0.95).to(torch.uint8)
    emap = torch.empty(shape, dtype=torch.uint8, device=dev)
    emask = torch.empty(shape, dtype=torch.uint8, device=dev)
    hist = torch.zeros(257, dtype=torch.int64, device=dev)
    res = {}
    for name, m in (("aff_errors_mask", mask), ("aff_errors_nomask", None)):
        ms = events(lambda: eng.aff_errors(seg, (0, 0, 0), pred, m, NHOOD, chunk, (0.1, 1.0), shape[0], emap, emask, hist))
        bpv = 8 + 6 + (1 if m is not None else 0) + 4 + 4 + 2
        res[name] = {"ms": ms, "bytes_per_voxel": bpv, "GBps": bpv * nv / ms / 1e6, "hbm_fraction": bpv * nv / ms / 1e-3 / HBM,
                     "ms_per_1e8_voxels": ms * 1e8 / nv}
    gt = voronoi_like(shape, (32, 128, 128), 2)
    segc = seg[: shape[0], : shape[1], : shape[2]].contiguous()
    out = torch.empty((3, eng.cap), dtype=torch.int64, device=dev)
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    st = eng.stream

    def pairs():
        _lib.check(_lib.lib.bsmi_eval_pairs_u64(eng.h, C.c_void_p(gt.data_ptr()), C.c_void_p(segc.data_ptr()), C.c_void_p(mask.data_ptr()),
                                                _lib.i64x3(shape), 1, st))
        _lib.check(_lib.lib.bsmi_eval_pairs_read(eng.h, C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()),
                                                 C.c_void_p(out[2].data_ptr()), eng.cap, C.c_void_p(n.data_ptr()), st))
    ms = events(pairs)
    _lib.check(_lib.lib.bsmi_eval_status(eng.h, st))
    bpv = 8 + 8 + 1
    res["pairs_mask"] = {"ms": ms, "bytes_per_voxel": bpv, "GBps": bpv * nv / ms / 1e6, "hbm_fraction": bpv * nv / ms / 1e-3 / HBM,
                         "pairs": int(n.item()), "table_clear_and_readout_bytes": eng.cap * 8 * 5}
    eng.close()
    return {"part": "device", "shape": list(shape), "chunk": list(chunk), "voxels": nv, **res}


def _ref_one(args):
    import eval_ref as R
    seg, pred, mask, gt = args
    t = time.perf_counter()
    emap, emask = R.aff_errors(seg, (0, 0, 0), pred, NHOOD, (32, 128, 128), mask=mask)
    t_err = time.perf_counter() - t
    t = time.perf_counter()
    voi = R.rand_voi(gt, seg, mask)
    return emap, emask, voi, t_err, time.perf_counter() - t


def e2e_part(shape=(64, 512, 512), n_segs=4):
    import concurrent.futures as cf
    from bootstrapper_amd.evaluate import run_evaluation
    from bootstrapper_amd.zarr_io import open_ds, prepare_ds
    rng = np.random.default_rng(3)
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR")) as tmp:
        store = os.path.join(tmp, "vol.zarr")
        pred = torch.randint(0, 256, (6,) + shape, dtype=torch.uint8, device=dev).cpu().numpy()
        gt = voronoi_like(shape, (16, 64, 64), 9).cpu().numpy().view(np.uint64)
        mask = (rng.random(shape) < 0.9).astype(np.uint8)
        def put(name, a, chunk):
            d = prepare_ds(f"{store}/{name}", a.shape, offset=(0, 0, 0), voxel_size=(40, 4, 4), chunk_shape=chunk, dtype=a.dtype,
                           axis_names=(["c^"] if a.ndim == 4 else []) + ["z", "y", "x"], units=["nm"] * 3)
            d[:] = a
        put("predictions/3d_affs", pred, (6, 32, 128, 128))
        put("labels", gt, (32, 128, 128))
        put("mask", mask, (32, 128, 128))
        segs = []
        for i in range(n_segs):
            s = voronoi_like(shape, (8 + 4 * i, 48 + 16 * i, 48 + 16 * i), 20 + i).cpu().numpy().view(np.uint64)
            put(f"segmentations/seg{i}", s, (32, 128, 128))
            segs.append(s)
        cfg = os.path.join(tmp, "04_eval_vol.toml")
        with open(cfg, "w") as f:
            f.write(f'seg_datasets_prefix = "{store}/segmentations"\nmask_dataset = "{store}/mask"\n[gt]\nlabels_dataset = "{store}/labels"\n'
                    f'[pred]\npred_dataset = "{store}/predictions/3d_affs"\n')
        walls = {}
        for mode in ("pred", "gt"):
            torch.cuda.synchronize()
            t = time.perf_counter()
            run_evaluation(cfg, mode)
            walls[mode] = time.perf_counter() - t
        res = {m: json.load(open(os.path.join(tmp, f"results_{m}_vol.json"))) for m in ("pred", "gt")}
        t = time.perf_counter()
        with cf.ProcessPoolExecutor(max_workers=min(16, n_segs)) as pool:
            refs = list(pool.map(_ref_one, [(s, pred, mask, gt) for s in segs]))
        t_ref = time.perf_counter() - t
        agree = True
        for i, (emap, emask, voi, _, _) in enumerate(refs):
            sp = f"{store}/segmentations/seg{i}"
            agree &= bool(np.array_equal(open_ds(sp + "__vs__3d_affs/error_map")[:], emap))
            agree &= bool(np.array_equal(open_ds(sp + "__vs__3d_affs/error_mask")[:], emask))
            agree &= all(abs(res["gt"][sp]["metrics"]["voi"][k] - v) <= 1e-12 * max(1, abs(v)) for k, v in voi.items())
        return {"part": "e2e", "shape": list(shape), "segmentations": n_segs, "voxels_per_seg": int(np.prod(shape)),
                "bs_evaluate_pred_s": walls["pred"], "bs_evaluate_gt_s": walls["gt"], "eval_ref_wall_s": t_ref,
                "eval_ref_processes": min(16, n_segs), "eval_ref_errors_s_per_seg": [r[3] for r in refs],
                "eval_ref_rand_voi_s_per_seg": [r[4] for r in refs], "outputs_agree": agree}


def lsd_part(cases=(((64, 1024, 1024), (8, 256, 256), True), ((256, 512, 512), (128, 128, 128), True),
                    ((256, 512, 512), (128, 128, 128), False)), e2e_shape=(64, 512, 512), n_segs=4):
    """cases: (ROI shape, chunk, ragged boundaries).  With ragged boundaries most cells of the 2x sub-sampled grid hold voxels
    of several objects, and the cell's statistics are computed once per object; with boxes nearly every cell holds one."""
    from bootstrapper_amd.evaluate import lsd_setup, run_evaluation
    from bootstrapper_amd.train import lsd_targets
    from bootstrapper_amd.zarr_io import prepare_ds
    vs = (40, 8, 8)
    lsd = lsd_setup(vs)
    m, ctx = lsd["margin"], lsd["context"]
    halo = [a + b for a, b in zip(m, ctx)]
    eng = EvalDevice(0)
    res = {}
    for shape, chunk, ragged in cases:
        nv = int(np.prod(shape))
        seg = voronoi_like([n + 2 * h for n, h in zip(shape, halo)], (16, 96, 96), 1, jitter=ragged)
        grown = [n + 2 * a for n, a in zip(shape, m)]
        pred = torch.randint(0, 256, [10] + grown, dtype=torch.uint8, device=dev)
        mask = (torch.rand(grown, device=dev) < 0.95).to(torch.uint8)
        emap = torch.empty(shape, dtype=torch.uint8, device=dev)
        emask = torch.empty(shape, dtype=torch.uint8, device=dev)
        hist = torch.zeros(257, dtype=torch.int64, device=dev)
        ms = events(lambda: eng.lsd_errors(seg, [-h for h in halo], pred, mask, shape, chunk, lsd, (0.1, 1.0), shape[0], emap, emask, hist))
        _lib.check(_lib.lib.bsmi_eval_status(eng.h, eng.stream))
        g = [c + 2 * a for c, a in zip(chunk, m)]
        chunks = int(np.prod([-(-n // c) for n, c in zip(shape, chunk)]))
        # the only earlier way to these descriptors: the training kernel on one chunk's grown label array
        L = [a + 2 * b for a, b in zip(g, ctx)]
        labels = seg[:L[0], :L[1], :L[2]].contiguous()
        ms_train = events(lambda: lsd_targets(labels, ctx, g, [80.0] * 3, vs, 2, None), reps=3)
        res["x".join(map(str, chunk)) + ("_ragged" if ragged else "_boxes")] = {
            "shape": list(shape), "voxels": nv, "chunks": chunks, "grown_voxels_per_chunk": int(np.prod(g)), "ms": ms,
            "ms_per_1e8_voxels": ms * 1e8 / nv, "train_lsd_targets_ms_one_chunk": ms_train,
            "train_lsd_targets_ms_per_1e8_voxels": ms_train * chunks * 1e8 / nv, "ratio": ms_train * chunks / ms,
            "error_mask_ones": int(hist[256].item())}
        del seg, pred, mask, labels
        torch.cuda.empty_cache()
    eng.close()
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR")) as tmp:
        store = os.path.join(tmp, "vol.zarr")
        def put(name, a, chunk):
            d = prepare_ds(f"{store}/{name}", a.shape, offset=(0, 0, 0), voxel_size=vs, chunk_shape=chunk, dtype=a.dtype,
                           axis_names=(["c^"] if a.ndim == 4 else []) + ["z", "y", "x"], units=["nm"] * 3)
            d[:] = a
        put("predictions/3d_lsds", torch.randint(0, 256, (10,) + e2e_shape, dtype=torch.uint8, device=dev).cpu().numpy(), (10, 32, 128, 128))
        put("mask", (np.random.default_rng(3).random(e2e_shape) < 0.9).astype(np.uint8), (32, 128, 128))
        for i in range(n_segs):
            put(f"segmentations/seg{i}", voronoi_like(e2e_shape, (8 + 4 * i, 48 + 16 * i, 48 + 16 * i), 20 + i).cpu().numpy().view(np.uint64),
                (32, 128, 128))
        cfg = os.path.join(tmp, "04_eval_vol.toml")
        with open(cfg, "w") as f:
            f.write(f'seg_datasets_prefix = "{store}/segmentations"\nmask_dataset = "{store}/mask"\n'
                    f'[pred]\npred_dataset = "{store}/predictions/3d_lsds"\n')
        walls = []
        for _ in range(2):   # the second run overwrites the first one's outputs: warm library, warm page cache
            torch.cuda.synchronize()
            t = time.perf_counter()
            run_evaluation(cfg, "pred", lsd_errors=True)
            walls.append(time.perf_counter() - t)
    return {"part": "lsd", "margin": m, "context": ctx, "sigma": 80, **res, "e2e_shape": list(e2e_shape), "e2e_segmentations": n_segs,
            "bs_evaluate_pred_lsd_s": walls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["device", "e2e", "lsd"])
    a = ap.parse_args()
    if a.only in (None, "device"):
        print(json.dumps(device_part()), flush=True)
        torch.cuda.empty_cache()
    if a.only in (None, "e2e"):
        print(json.dumps(e2e_part()), flush=True)
        torch.cuda.empty_cache()
    if a.only in (None, "lsd"):
        print(json.dumps(lsd_part()), flush=True)


if __name__ == "__main__":
    main()
