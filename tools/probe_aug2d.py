"""Dev tool: the geometric and the intensity augmentation of the 2-D setups on one GPU -> JSON lines.

launches device-event ms of each of the four launches (after a warm-up, median of 9) at the shipped 2d_mtlsd shape: S = 10
         draws, K = 3 sections, input 196 x 196, output 104 x 104, an LSD context of 60 pixels at voxel size (40, 4, 4), so a
         frame of 224 x 224: aug2d_coords for ten full plans (lattice + shifts; including its three small uploads), raw over
         the input section, labels and mask over the labels window; with the bytes each launch must move and the rate that
         makes.
intensity  the batched intensity chain at the same shape (ten plans that apply every node, sigma 1.5): device-event ms of each
         launch and of the whole chain (median of 9), next to TEN calls of augment.apply_intensity on the ten stacks, the only way
         to the same result without the batched launches.
source   batches/s of SectionSource alone on a synthetic Zarr store written here: plain, `augment2d`, and `augment2d` with
         `intensity = true`, wall clock.
train    steps/s of a Trainer of the same setup fed through PrefetchSource: plain once, then `augment2d` and `augment2d` +
         intensity alternating twice, and how long the trainer waited for batches in each.
`--only launches|intensity|source|train`; `--batches N` (default 40)."""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from bootstrapper_amd import augment2d as A
from bootstrapper_amd.train import PrefetchSource, default_init, make_sample_source, training_settings

S, K, INPUT, OUTPUT, VOXEL = 10, 3, (196, 196), (104, 104), (40, 4, 4)
NET = {"in_channels": 1, "adj_slices": K, "num_fmaps": 12, "fmap_inc_factor": 5, "downsample_factors": [[2, 2]] * 3,
       "kernel_size_down": [[[3, 3], [3, 3]]] * 4, "kernel_size_up": [[[3, 3], [3, 3]]] * 3,
       "input_shape": list(INPUT), "output_shape": list(OUTPUT), "inputs": {"raw": {"dims": 1}},
       "outputs": {"2d_lsds": {"dims": 6, "sigma": 80, "downsample": 2},
                   "2d_affs": {"dims": 6, "neighborhood": [[-1, 0], [0, -1], [-9, 0], [0, -9], [-27, 0], [0, -27]], "grow_boundary": 1}}}


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
    margin = (60, 60)
    frame = A.frame_of(INPUT, OUTPUT, margin, margin)
    plans = [A.draw_plan2d(rng, A.Aug2DParams(deform_p=1.0), INPUT, frame, K, VOXEL) for _ in range(S)]
    packed = A.Packed2D(plans, [A.source_box2d(p) for p in plans])
    raw = torch.randint(0, 256, (K * packed.crop_pixels,), dtype=torch.uint8, device="cuda")
    lab = torch.randint(1, 1 << 40, (packed.crop_pixels,), dtype=torch.int64, device="cuda")
    mask = torch.randint(0, 2, (packed.crop_pixels,), dtype=torch.uint8, device="cuda")
    ctx = [(i - o) // 2 for i, o in zip(INPUT, OUTPUT)]
    window = ([c - m for c, m in zip(ctx, margin)], [o + 2 * m for o, m in zip(OUTPUT, margin)])
    section = ((0, 0), INPUT)
    n_frame, n_in, n_win = S * K * int(np.prod(packed.frame_shape)), S * K * int(np.prod(INPUT)), S * int(np.prod(window[1]))
    coords = A.coords2d(packed, 0)
    ms = {"coords": events(lambda: A.coords2d(packed, 0)), "raw": events(lambda: A.sample_raw2d(packed, coords, raw, section)),
          "labels": events(lambda: A.sample_labels2d(packed, coords, lab, window)), "mask": events(lambda: A.sample_mask2d(packed, coords, mask, window))}
    # bytes a launch cannot avoid: the coordinate planes, one gather per corner or sample (counted at its own size, not the
    # sector it drags in), the output.  coords also includes its small uploads (table, lattices, shifts) in the timed call.
    need = {"coords": 8 * n_frame, "raw": (8 + 4 + 4) * n_in, "labels": (8 + 8 + 8) * n_win, "mask": (8 + 1 + 1) * n_win}
    return {"part": "launches", "frame": list(packed.frame_shape), "crops": [list(c) for c in packed.crop_shapes],
            "lattice": list(plans[0].lattice.shape[1:]), "window": window[1], "ms": ms, "needed_MB": {k: v / 1e6 for k, v in need.items()},
            "GB_per_s": {k: need[k] / ms[k] / 1e6 for k in ms}}


def intensity_part():
    from bootstrapper_amd import augment as G
    rng = np.random.default_rng(0)
    shape = (K,) + INPUT
    lo, hi = G.gamma_interval((0.8, 1.2))
    plans = [G.IntensityPlan(shape, noise_sigma=float(np.float32(0.1)), scale=rng.uniform(0.9, 1.1, K).astype(np.float32),
                             shift=rng.uniform(-0.1, 0.1, K).astype(np.float32), gamma=G.gamma_exponent(rng.uniform(lo, hi, K)).astype(np.float32),
                             impulse_threshold=2 ** 31, blur=1.5, weights=G.gaussian_weights(1.5), defect=np.array([3, 0, 0], dtype=np.int32),
                             seed=int(rng.integers(0, 2 ** 64, dtype=np.uint64))) for _ in range(S)]
    t = A.PackedIntensity2D(plans)
    x0 = torch.rand((K, S) + INPUT, dtype=torch.float32, device="cuda")
    x = x0.clone()
    t.upload(x.device)
    st, tmp = A.plane_stats(x), torch.empty_like(x)
    ms = {"noise": events(lambda: A.noise2d(x, t)), "stats": events(lambda: A.plane_stats(x)), "intensity": events(lambda: A.intensity2d(x, t, st)),
          "gamma": events(lambda: A.gamma2d(x, t, st)), "impulse": events(lambda: A.impulse2d(x, t)), "smooth": events(lambda: A.smooth2d(x, t, tmp)),
          "defect": events(lambda: A.defect2d(x, t, st, True))}
    stacks = [x0[:, s].contiguous() for s in range(S)]

    def ten_calls():
        for s in range(S):
            G.apply_intensity(stacks[s], plans[s])

    def fresh():   # the descriptor, per-plane and taps uploads are part of a batch's chain
        return A.apply_intensity2d(x, A.PackedIntensity2D(plans))
    chain = {"batched_chain": events(lambda: A.apply_intensity2d(x, t)), "batched_chain_with_packing_and_uploads": events(fresh),
             "ten_calls_of_apply_intensity": events(ten_calls)}
    return {"part": "intensity", "voxels": int(x.numel()), "launch_ms": ms, "chain_ms": chain,
            "speedup_over_ten_calls": chain["ten_calls_of_apply_intensity"] / chain["batched_chain_with_packing_and_uploads"]}


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


SOURCES = (("plain", False), ("augment2d", True), ("augment2d+intensity", {"intensity": True}))


def source_part(cfg, batches):
    res = {"part": "source", "batches": batches}
    for name, aug in SOURCES:
        src = make_sample_source(dict(cfg, augment2d=aug), NET, 0, 0)
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
    for name, aug in SOURCES + SOURCES[1:]:   # alternating: the spread shows
        src = PrefetchSource(make_sample_source(dict(cfg, augment2d=aug), NET, 0, 0), 4, 0)
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
    ap.add_argument("--only", choices=["launches", "intensity", "source", "train"])
    ap.add_argument("--batches", type=int, default=40)
    a = ap.parse_args()
    if a.only in (None, "launches"):
        print(json.dumps(launches_part()), flush=True)
    if a.only in (None, "intensity"):
        print(json.dumps(intensity_part()), flush=True)
    if a.only in (None, "source", "train"):
        with tempfile.TemporaryDirectory() as root:
            cfg = write_store(root)
            if a.only in (None, "source"):
                print(json.dumps(source_part(cfg, a.batches)), flush=True)
            if a.only in (None, "train"):
                print(json.dumps(train_part(cfg, a.batches)), flush=True)


if __name__ == "__main__":
    main()
