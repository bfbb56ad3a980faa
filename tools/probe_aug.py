"""Dev tool: the training augmentation, geometric and intensity, on one GPU -> JSON lines.

launches device-event ms of each launch (after a warm-up, median of 9) at the 3d_mtlsd shape, input (32, 196, 196), output
         (4, 104, 104): aug_coords for a full plan (lattice + shifts), raw over the input block, labels and mask over the
         output block grown by the LSD context; with the bytes each launch must move and the rate that makes.  Then a leg
         per launch of the intensity chain on the input block: unit resampling, noise, section statistics (its two
         launches), intensity, gamma, impulse, smooth (z pass and y/x pass together, sigma 1.5), defect, and the whole
         chain of a plan that applies every node.
source   batches/s of SampleSource alone on a synthetic Zarr store written here: plain, `augment`, `augment` with
         `intensity`, wall clock.
train    steps/s of a Trainer of the same setup fed through PrefetchSource with each of the three, alternating, and how long
         the trainer waited for batches in each.
The store is at voxel size (40, 8, 8) with an LSD sigma of 80: at (40, 4, 4) the descriptors' context (60 voxels) exceeds the
network's (46), which the augmented source refuses.  `--only launches|source|train`; `--batches N` (default 40)."""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from bootstrapper_amd import augment as A
from bootstrapper_amd.train import PrefetchSource, default_init, make_sample_source, training_settings

INPUT, OUTPUT, VOXEL = (32, 196, 196), (4, 104, 104), (40, 8, 8)
NET = {"in_channels": 1, "num_fmaps": 12, "fmap_inc_factor": 5, "downsample_factors": [[1, 2, 2]] * 3,
       "kernel_size_down": [[[3, 3, 3], [3, 3, 3]]] * 4, "kernel_size_up": [[[3, 3, 3], [3, 3, 3]]] * 3,
       "input_shape": list(INPUT), "output_shape": list(OUTPUT),
       "outputs": {"3d_lsds": {"dims": 10, "sigma": 80, "downsample": 2},
                   "3d_affs": {"dims": 3, "neighborhood": [[-1, 0, 0], [0, -1, 0], [0, 0, -1]], "grow_boundary": 1}}}


def events(fn, reps=9):
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


def launches_part():
    rng = np.random.default_rng(0)
    plan = A.draw_plan(rng, A.AugParams(deform_p=1.0, shift_p=1.0), INPUT, VOXEL)
    lo, hi = A.source_box(plan)
    size = tuple(h - l for l, h in zip(lo, hi))
    raw = torch.randint(0, 256, size, dtype=torch.uint8, device="cuda")
    lab = torch.randint(1, 1 << 40, size, dtype=torch.int64, device="cuda")
    mask = torch.randint(0, 2, size, dtype=torch.uint8, device="cuda")
    ctx = [(i - o) // 2 for i, o in zip(INPUT, OUTPUT)]
    cv = (6, 30, 30)
    region = ([c - v for c, v in zip(ctx, cv)], [o + 2 * v for o, v in zip(OUTPUT, cv)])
    n_in, n_reg = int(np.prod(INPUT)), int(np.prod(region[1]))
    coords = A.coords(plan, lo, 0)
    ms = {"coords": events(lambda: A.coords(plan, lo, 0)), "raw": events(lambda: A.sample_raw(coords, raw)),
          "labels": events(lambda: A.sample_labels(coords, lab, region)), "mask": events(lambda: A.sample_mask(coords, mask, region))}
    # bytes a launch cannot avoid: the coordinate planes, one gather per corner or sample (counted at its own size, not the
    # sector it drags in), the output.  coords also includes its two small uploads (lattice, shifts) in the timed call.
    need = {"coords": 12 * n_in, "raw": (12 + 8 + 4) * n_in, "labels": (12 + 8 + 8) * n_reg, "mask": (12 + 1 + 1) * n_reg}
    # the intensity chain: every node on the input block, in place (values stay in [0, 1] whatever the repeat count)
    x = A.sample_unit(coords, raw)
    d = INPUT[0]
    sec = np.random.default_rng(1)
    scale, shift = [torch.from_numpy(sec.uniform(lo_, hi_, d).astype(np.float32)).cuda() for lo_, hi_ in ((0.9, 1.1), (-0.1, 0.1))]
    expo = torch.from_numpy(sec.uniform(0.8, 1.2, d).astype(np.float32)).cuda()
    mode = torch.from_numpy((np.arange(d) % 4).astype(np.int32)).cuda()
    weights = A.gaussian_weights(1.5)
    st = A.section_stats(x)
    full = A.IntensityPlan(INPUT, noise_sigma=0.1, scale=scale.cpu().numpy(), shift=shift.cpu().numpy(), gamma=expo.cpu().numpy(),
                           impulse_threshold=2 ** 31, blur=1.5, weights=weights, defect=mode.cpu().numpy(), seed=7)
    ims = {"unit": events(lambda: A.sample_unit(coords, raw)), "noise": events(lambda: A.noise(x, 7, 0.1)),
           "stats": events(lambda: A.section_stats(x)), "intensity": events(lambda: A.intensity(x, st, scale, shift)),
           "gamma": events(lambda: A.gamma(x, st, expo)), "impulse": events(lambda: A.impulse(x, 7, 2 ** 31)),
           "smooth": events(lambda: A.smooth(x, weights)), "defect": events(lambda: A.defect(x, st, mode, 0.1, True)),
           "chain": events(lambda: A.apply_intensity(x, full, final_map=False))}
    ms.update({"intensity_" + k: v for k, v in ims.items()})
    # read + write of the block; stats reads it once; smooth reads and writes it twice; the chain: 3 statistics and 7 passes
    need.update({"intensity_" + k: v * n_in for k, v in {"unit": 12 + 8 + 4, "noise": 8, "stats": 4, "intensity": 8, "gamma": 8, "impulse": 8,
                                                           "smooth": 16, "defect": 8, "chain": 3 * 4 + 7 * 8}.items()})
    return {"part": "launches", "crop": list(size), "lattice": list(plan.lattice.shape[1:]), "region": region[1], "ms": ms,
            "needed_MB": {k: v / 1e6 for k, v in need.items()}, "GB_per_s": {k: need[k] / ms[k] / 1e6 for k in ms}}


def write_store(root):
    from bootstrapper_amd.zarr_io import prepare_ds
    shape = (64, 512, 512)
    rng = np.random.default_rng(1)
    raw = rng.integers(0, 256, size=shape, dtype=np.uint8)
    ids = rng.integers(1, 1 << 20, size=(8, 16, 16)).astype(np.uint64)
    labels = np.repeat(np.repeat(np.repeat(ids, 8, 0), 32, 1), 32, 2)
    for name, arr in (("raw", raw), ("labels", labels)):
        ds = prepare_ds(f"{root}/vol.zarr/{name}", arr.shape, offset=(0, 0, 0), voxel_size=VOXEL, chunk_shape=(32, 128, 128), dtype=arr.dtype)
        ds[:] = arr
    return {"samples": [{"raw": f"{root}/vol.zarr/raw", "labels": f"{root}/vol.zarr/labels"}], "voxel_size": list(VOXEL)}


def source_part(cfg, batches):
    res = {"part": "source", "batches": batches}
    for name, aug in (("plain", False), ("augment", True), ("augment + intensity", {"intensity": True})):
        src = make_sample_source(dict(cfg, augment=aug), NET, 0, 0)
        next(src)
        torch.cuda.synchronize()
        per = []
        for _ in range(batches):
            t = time.perf_counter()
            next(src)
            torch.cuda.synchronize()
            per.append(time.perf_counter() - t)
        res[name] = {"batches_per_s": batches / sum(per), "ms_median": 1e3 * float(np.median(per)), "ms_max": 1e3 * max(per)}
    return res


def train_part(cfg, batches):
    from bootstrapper_amd.training import Trainer
    from bootstrapper_amd.unet import Model
    model = Model(NET, device=0, precision="f32")
    model.load_state_dict(default_init(NET, seed=42))
    settings = training_settings(NET)
    trainer = Trainer(model, settings["in_shape"], lr=settings["lr"])
    res = {"part": "train", "steps": batches, "runs": []}
    three = (("plain", False), ("augment", True), ("augment + intensity", {"intensity": True}))
    for name, aug in three + three:   # alternating: the spread shows
        src = PrefetchSource(make_sample_source(dict(cfg, augment=aug), NET, 0, 0), 4, 0)
        try:
            for _ in range(3):
                trainer.training_step(next(src))
            torch.cuda.synchronize()
            waited, t = 0.0, time.perf_counter()
            for _ in range(batches):
                w = time.perf_counter()
                batch = next(src)
                waited += time.perf_counter() - w
                trainer.training_step(batch)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t
        finally:
            src.close()
        res["runs"].append({"source": name, "steps_per_s": batches / wall, "waited_for_batches_s": waited, "wall_s": wall})
    trainer.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["launches", "source", "train"])
    ap.add_argument("--batches", type=int, default=40)
    a = ap.parse_args()
    if a.only in (None, "launches"):
        print(json.dumps(launches_part()), flush=True)
    if a.only in (None, "source", "train"):
        with tempfile.TemporaryDirectory() as root:
            cfg = write_store(root)
            if a.only in (None, "source"):
                print(json.dumps(source_part(cfg, a.batches)), flush=True)
            if a.only in (None, "train"):
                print(json.dumps(train_part(cfg, a.batches)), flush=True)


if __name__ == "__main__":
    main()
