"""Dev tool: `bs predict` on an on-disk Zarr store of the synthetic volume (the predict half of bench.py's `drivers` leg, as
tools/probe_drivers.py sets it up) with BSMI_IO_TRACE=1, alternating BSMI_PRED_DEVICE_FRAMES=0 and 1 in one session: wall time of
the command and the trace's "block loop" / "waits for a writer" lines per run.  The two datasets of the last pair are compared.
python tools/probe_pred_frames.py [edge_blocks] [pairs]"""
import json
import os
import shutil
import sys
import tempfile
import time

os.environ.setdefault("BSMI_IO_TRACE", "1")
os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from bootstrapper_amd.predict import run_prediction
from bootstrapper_amd.synth import synthetic_state_dict, synthetic_volume
from bootstrapper_amd.zarr_io import open_ds, prepare_ds

edge = int(sys.argv[1]) if len(sys.argv) > 1 else 8
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 2
print(torch.cuda.get_device_name(0), flush=True)
sd = synthetic_state_dict(bench.NET_CONFIG, 0)
vol = synthetic_volume((128 * edge,) * 3, seed=0, device=torch.device("cuda", 0)).cpu().numpy()
torch.cuda.empty_cache()
tmp = tempfile.mkdtemp(prefix="bsmi_pred_frames_", dir=os.environ.get("BSMI_BENCH_TMP"))
try:
    setup = os.path.join(tmp, "3d_affs")
    os.makedirs(setup)
    nc = dict(bench.NET_CONFIG, input_shape=[o + 2 * c for o, c in zip(bench.OUT_BLOCK, bench.CONTEXT)], output_shape=list(bench.OUT_BLOCK),
              shape_increase=[0, 0, 0], inputs={"raw": {"dims": 1}}, outputs={"3d_affs": {"dtype": "uint8", "dims": 6}})
    with open(os.path.join(setup, "net_config.json"), "w") as f:
        json.dump(nc, f)
    ckpt = os.path.join(setup, "model_checkpoint_1")
    torch.save({"model_state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}, ckpt + ".ckpt")
    store = os.path.join(tmp, "vol.zarr")
    ds = prepare_ds(store + "/raw", vol.shape, offset=(0, 0, 0), voxel_size=(1, 1, 1), chunk_shape=bench.OUT_BLOCK, dtype=np.uint8,
                    axis_names=["z", "y", "x"], units=["nm"] * 3)
    ds[:] = vol
    blocks = edge ** 3
    kept = {}
    for rep in range(2 * pairs):
        switch = str(rep % 2)
        os.environ["BSMI_PRED_DEVICE_FRAMES"] = switch
        prefix = f"{store}/pred_{switch}"
        shutil.rmtree(prefix, ignore_errors=True)
        toml = os.path.join(tmp, f"pred_{switch}.toml")
        with open(toml, "w") as f:
            f.write(f'["01-3d_affs"]\nsetup_dir = "{setup}"\ninput_datasets = ["{store}/raw"]\ncheckpoint = "{ckpt}"\n'
                    f'output_datasets_prefix = "{prefix}"\nchain_str = ""\nnum_workers = 1\nnum_gpus = 1\n')
        print(f"--- run {rep}: BSMI_PRED_DEVICE_FRAMES={switch}", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        run_prediction(toml, "01", precision="bf16x3")
        dt = time.perf_counter() - t0
        path = f"{prefix}/1/3d_affs"
        size = sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))
        print(f"run {rep}: BSMI_PRED_DEVICE_FRAMES={switch}: bs predict {dt:.3f} s, {1e3 * dt / blocks:.2f} ms per block of {blocks}, dataset {size / 1e6:.1f} MB on disk",
              flush=True)
        kept[switch] = path
    a, b = open_ds(kept["0"]), open_ds(kept["1"])
    differ = 0
    for z in range(0, a.shape[1], 128):
        differ += int(not np.array_equal(a[:, z:z + 128], b[:, z:z + 128]))
    print(f"datasets of the last pair: {differ} of {a.shape[1] // 128} slabs differ", flush=True)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
