"""Dev tool: the synthetic-label source of the second-stage setups on one GPU -> JSON lines.

stages   device-event ms per stage (after a warm-up, median of 5) at the reference shape: labels of (24, 148, 148) at
         anisotropy 10, i.e. a generated volume of 240 x 148 x 148: dilate, label, expand, label again (the tubes branch),
         gaussian, argmax filter, basins (the random branch), finish, grow_boundary, one split / merge / artifact, and the
         target calls of a 3d_affs_from_2d_mtlsd batch.
source   batches/s of SyntheticSource alone (its own draws: the branches and anisotropies as they come), wall clock.
train    steps/s of a training run of the same setup fed by that source through the prefetch thread, wall clock, and how
         long the trainer waited for batches.
augin    the input augmentation (`input_augment`): device-event ms per launch and per array (every node
         applied) at the two shipped input arrays, (6, 24, 148, 148) and (10, 24, 148, 148); then batches/s of the source and
         steps/s of the fed trainer without the key, with it, and without it again, in this one session.
labelaug the geometric augmentation of the labels (`label_augment`) at the shipped block (24, 148, 148):
         device-event ms of the pad, the coordinate launch and the resampling launch, and of warp_labels as a whole (with the plan's
         uploads); then batches/s of the source and steps/s of the fed trainer without the key, with it, and without it again, in
         this one session.
`--only stages|source|train|augin|labelaug`; `--batches N` (default 20)."""
import argparse, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from bootstrapper_amd import synth_labels as S
from bootstrapper_amd.train import PrefetchSource, SyntheticSource, affinity_targets_roi, default_init, lsd2d_targets, training_settings

SHAPE, ANISO, VOXEL = (24, 148, 148), 10, (40, 4, 4)


def net_config():
    """the 3d_affs_from_2d_mtlsd setup as the family golden holds it (input (24, 148, 148), output (4, 56, 56), 6 + 6 input
    channels, 9 affinities), at the setup's full widths"""
    d = np.load(os.path.join(ROOT, "tests", "golden", "family_from_2d_mtlsd_f3i2.npz"))
    return dict(json.loads(bytes(d["net_config"]).decode()), num_fmaps=9, num_fmaps_out=18, fmap_inc_factor=3)


NET = net_config()


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


def tubes_plan(seed=0):
    """the first plan of the stream that is a tubes plan at anisotropy 10"""
    for s in range(seed, seed + 10000):
        p = S.draw_plan(random.Random(s), SHAPE, (ANISO, ANISO))
        if p.choice == "tubes":
            return p
    raise RuntimeError("no tubes plan")


def stages_part():
    eng = S.SynthEngine((SHAPE[0] * ANISO,) + SHAPE[1:], 0)
    p = tubes_plan()
    gen = p.generated_shape
    res = {}
    res["dilate"] = events(lambda: eng.dilate_points(gen, p.points, p.structs, p.struct_index, p.dilations))
    fg = eng.dilate_points(gen, p.points, p.structs, p.struct_index, p.dilations)
    res["label_binary"] = events(lambda: eng.label(fg))
    lab, n = eng.label(fg)
    res["expand"] = events(lambda: eng.expand(lab, gen[0], n + 1))
    ex = eng.expand(lab, gen[0], n + 1)
    res["label_expanded"] = events(lambda: eng.label(ex))
    res["tubes_all"] = events(lambda: eng.tubes(fg))
    tub = eng.tubes(fg)[0]
    noise = torch.rand(gen, dtype=torch.float32, device="cuda")
    res["gaussian"] = events(lambda: eng.gaussian(noise))
    peaks = eng.gaussian(noise)
    res["argmax_filter"] = events(lambda: eng.argmax_filter(peaks))
    pos = eng.argmax_filter(peaks)
    res["basins"] = events(lambda: eng.basins(peaks, pos))
    res["random_all"] = events(lambda: eng.random_labels(noise))
    res["finish"] = events(lambda: eng.finish(tub, True, False, ANISO))
    labels = eng.finish(tub, False, False, ANISO)
    res["grow_boundary"] = events(lambda: eng.grow_boundary(labels, 7, 1))
    grown = eng.grow_boundary(labels, 7, 1)
    ids = eng.present(grown)
    res["present"] = events(lambda: eng.present(grown))
    res["split"] = events(lambda: eng.split(grown.clone(), ids[len(ids) // 2], 30, [3, 11], max(ids)))
    res["merge"] = events(lambda: eng.merge(grown.clone(), [3, 11], ids[0], ids[-1]))
    res["artifact"] = events(lambda: eng.stamp(grown.clone(), 5, 20, 30, S.star(8), max(ids) + 1))
    res["clone_only"] = events(lambda: grown.clone())
    src = SyntheticSource(NET, VOXEL, 0)
    for key, spec in src.inputs:
        res[f"input_{key}"] = events(lambda: src._input(key, spec, grown))
    ctx = [(i - o) // 2 for i, o in zip(src.inp, src.out)]
    res["gt_affs"] = events(lambda: affinity_targets_roi(grown[None].contiguous(), None, ctx, src.out, src.out_nhood, src.out_grow, only_xy=True))
    eng.close()
    return {"part": "stages", "generated_shape": list(gen), "labels_in_volume": len(ids), "ms": res}


def source_part(batches, input_augment=None, label_augment=None):
    src = SyntheticSource(NET, VOXEL, 0, seed=42, input_augment=input_augment, label_augment=label_augment)
    next(src)
    torch.cuda.synchronize()
    per = []
    for _ in range(batches):
        t = time.perf_counter()
        next(src)
        torch.cuda.synchronize()
        per.append(time.perf_counter() - t)
    return {"part": "source", "input_augment": input_augment is not None, "label_augment": label_augment is not None, "batches": batches, "batches_per_s": batches / sum(per), "ms_median": 1e3 * float(np.median(per)),
            "ms_min": 1e3 * min(per), "ms_max": 1e3 * max(per)}


def make_trainer():
    from bootstrapper_amd.training import Trainer
    from bootstrapper_amd.unet import Model
    model = Model(NET, device=0, precision="f32")
    model.load_state_dict(default_init(NET, seed=42))
    settings = training_settings(NET)
    return Trainer(model, settings["in_shape"], lr=settings["lr"])


def fed(trainer, batches, input_augment=None, label_augment=None):
    """steps/s of `trainer` fed by the source through the prefetch thread, wall clock, and how long it waited for batches"""
    src = PrefetchSource(SyntheticSource(NET, VOXEL, 0, seed=42, input_augment=input_augment, label_augment=label_augment), 4, 0)
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
    return {"input_augment": input_augment is not None, "label_augment": label_augment is not None, "fed_steps_per_s": batches / wall, "waited_for_batches_s": waited, "wall_s": wall}


def augin_part(batches):
    from bootstrapper_amd import augment_inputs as A
    res = {"part": "augin", "launch_ms": {}, "source": [], "train": []}
    for shape in ((6,) + SHAPE, (10,) + SHAPE):
        c, d = shape[:2]
        x = torch.rand(shape, dtype=torch.float32, device="cuda")
        rng = np.random.default_rng(1)
        on = A.InputAugParams(noise_p=1.0, channel_intensity_p=1.0, section_intensity_p=1.0, smooth_p=1.0, blur=(0.5, 1.5), prob_low_contrast=1.0)
        plan = A.draw_input_plan(rng, on, shape)
        t = {k: torch.from_numpy(getattr(plan, k)).cuda() for k in ("channel_scale", "channel_shift", "section_scale", "section_shift", "weights",
                                                                     "radius", "low_contrast")}
        mc, mz = A.group_mean(x, 0), A.group_mean(x, 1)
        res["launch_ms"]["x".join(str(v) for v in shape)] = {
            "noise": events(lambda: A.noise(x, plan.seed, plan.noise_sigma)),
            "group_mean_channel": events(lambda: A.group_mean(x, 0)),
            "group_mean_section": events(lambda: A.group_mean(x, 1)),
            "intensity_channel": events(lambda: A.intensity(x, mc, t["channel_scale"], t["channel_shift"], 0)),
            "intensity_section": events(lambda: A.intensity(x, mz, t["section_scale"], t["section_shift"], 1)),
            "smooth": events(lambda: A.smooth(x, t["weights"], t["radius"], True)),
            "smooth_plane_only": events(lambda: A.smooth(x, t["weights"], t["radius"], False)),
            "contrast": events(lambda: A.contrast(x, mz, t["low_contrast"], 0.1)),
            "array_every_node": events(lambda: A.apply_inputs(x, plan)),
            "voxels": int(x.numel()), "sections_smoothed": int((plan.radius > 0).sum()), "channels": c, "sections": d}
    params = A.InputAugParams()
    for key in (None, params, None):     # plain and augmented runs alternating in one session
        res["source"].append({k: v for k, v in source_part(batches, key).items() if k != "part"})
    trainer = make_trainer()
    for key in (None, params, None):
        res["train"].append(fed(trainer, batches, key))
    trainer.close()
    return res


def labelaug_part(batches):
    from bootstrapper_amd import augment as G
    from bootstrapper_amd import augment_labels as A
    params = A.LabelAugParams()
    on = A.LabelAugParams(shift_p=1.0)     # every node applied
    plan = G.draw_plan(np.random.default_rng(1), on.to_aug_params(VOXEL), SHAPE, VOXEL)
    lab = torch.randint(1, 2 ** 40, SHAPE, dtype=torch.int64, device="cuda")
    pad = lambda: torch.nn.functional.pad(lab, (1, 1, 1, 1, 1, 1)).contiguous()  # noqa: E731
    padded, coords = pad(), G.coords(plan, (-1, -1, -1), 0)
    res = {"part": "labelaug", "voxels": int(lab.numel()), "lattice_nodes": int(np.prod(plan.lattice.shape[1:])),
           "outside_share": float((A.warp_labels(lab, plan) == 0).float().mean()),
           "ms": {"pad": events(pad), "coords_with_uploads": events(lambda: G.coords(plan, (-1, -1, -1), 0)),
                  "sample_labels": events(lambda: G.sample_labels(coords, padded)), "warp_labels": events(lambda: A.warp_labels(lab, plan))},
           "source": [], "train": []}
    for key in (None, params, None):     # plain and augmented runs alternating in one session
        res["source"].append({k: v for k, v in source_part(batches, label_augment=key).items() if k != "part"})
    trainer = make_trainer()
    for key in (None, params, None):
        res["train"].append(fed(trainer, batches, label_augment=key))
    trainer.close()
    return res


def train_part(batches):
    trainer = make_trainer()
    res = {"part": "train", "steps": batches}
    # the trainer alone: one batch fed again and again
    one = next(SyntheticSource(NET, VOXEL, 0, seed=42))
    for _ in range(3):
        trainer.training_step(one)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(batches):
        trainer.training_step(one)
    torch.cuda.synchronize()
    res["trainer_alone_steps_per_s"] = batches / (time.perf_counter() - t)
    # fed by the source through the prefetch thread
    f = fed(trainer, batches)
    trainer.close()
    res.update(fed_steps_per_s=f["fed_steps_per_s"], waited_for_batches_s=f["waited_for_batches_s"], wall_s=f["wall_s"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["stages", "source", "train", "augin", "labelaug"])
    ap.add_argument("--batches", type=int, default=20)
    a = ap.parse_args()
    for name, fn in (("stages", stages_part), ("source", lambda: source_part(a.batches)), ("train", lambda: train_part(a.batches)),
                     ("augin", lambda: augin_part(a.batches)), ("labelaug", lambda: labelaug_part(a.batches))):
        if a.only in (None, name):
            print(json.dumps(fn()), flush=True)


if __name__ == "__main__":
    main()
