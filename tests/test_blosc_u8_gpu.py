"""csrc/blosc_dev_u8.hip: every frame that `bsmi_blosc_encode_dev_u8` makes here is byte-equal to the sequential restatement of
its rule (tests/blosc_u8_ref.py `encode_frame_ref`), reads back through the strict reader and the host codec, and leaves every
byte beyond the sizes that `bsmi_blosc_dev_u8_frame_bound` / `_scratch_bytes` promise untouched.  Chunk shapes of one block, a
block plus a short one, 105 bytes and four blocks; the byte cases of the CPU test; extents that overhang; a strided source; 1, 7
and 9 chunks per call; every refusal.  Every case asserts that it reached the edge it is named for.  Then `predict_blocks` with
the path on and off.  Needs an MI355X."""
import ctypes as C
import functools
import json
import os
import time

import numpy as np
import pytest
import torch

import blosc_ref as R
import blosc_u8_ref as U

pytestmark = pytest.mark.gpu

PAD = 4096      # bytes allocated beyond what the size functions promise, per slot and behind the scratch
FILL = 0xA5


@functools.lru_cache(maxsize=None)
def _cases():
    return U.byte_cases()


@functools.lru_cache(maxsize=None)
def _ref_frame(data):
    return U.encode_frame_ref(np.frombuffer(data, np.uint8))


def _call(src, strides, n, origins, extents, chunk, scratch, ns, frames, slot, sizes):
    from bootstrapper_amd import _lib
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)
    arr = lambda v: (C.c_int64 * len(v))(*v) if v is not None else None
    return _lib.lib.bsmi_blosc_encode_dev_u8(0, ptr(src), arr(strides), n, arr(origins), arr(extents), arr(chunk), ptr(scratch), ns, ptr(frames), slot,
                                             ptr(sizes), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _buffers(n, chunk_bytes):
    from bootstrapper_amd import _lib
    slot = int(_lib.lib.bsmi_blosc_dev_u8_frame_bound(chunk_bytes))
    ns = int(_lib.lib.bsmi_blosc_dev_u8_scratch_bytes(n, chunk_bytes))
    return (slot, ns, torch.full((ns + PAD,), FILL, dtype=torch.uint8, device="cuda"),
            torch.full((n * (slot + PAD),), FILL, dtype=torch.uint8, device="cuda"), torch.full((n * 4 + PAD,), FILL, dtype=torch.uint8, device="cuda"))


def _expected(host, g, chunk):
    out = np.zeros(chunk, np.uint8)
    part = host[tuple(slice(o, min(o + c, s)) for o, c, s in zip(g, chunk, host.shape))]
    out[tuple(slice(0, s) for s in part.shape)] = part
    return out


def _checked(host, chunk, src=None):
    """encode every chunk of the 4-D uint8 array `host` (from the device tensor `src`, by default a contiguous copy) into
    sentinel-filled slots and scratch; hold every frame against the restatement, the strict reader and the host codec, and every
    byte beyond the promised sizes against the sentinel -> [(grid index, frame)]"""
    from bootstrapper_amd import _lib, codecs
    if src is None:
        src = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    assert tuple(src.shape) == host.shape and src.stride(3) == 1
    grid = [(c, z, y, x) for c in range(0, host.shape[0], chunk[0]) for z in range(0, host.shape[1], chunk[1])
            for y in range(0, host.shape[2], chunk[2]) for x in range(0, host.shape[3], chunk[3])]
    n, cb = len(grid), int(np.prod(chunk))
    slot, ns, scratch, frames, sizes = _buffers(n, cb)
    origins = [v for g in grid for v in g]
    extents = [min(c, s - o) for g in grid for o, c, s in zip(g, chunk, host.shape)]
    _lib.check(_call(src, src.stride()[:3], n, origins, extents, chunk, scratch, ns, frames, slot + PAD, sizes))
    # (the ctypes arrays of the geometry died with `_call`: the call has read them, nothing of the caller's has to outlive it)
    torch.cuda.synchronize()
    assert (sizes[4 * n:].cpu().numpy() == FILL).all(), "frame sizes were written beyond the n-th"
    sz = sizes[:4 * n].cpu().numpy().view(np.uint32)
    fr = frames.cpu().numpy().reshape(n, slot + PAD)
    assert (scratch[ns:].cpu().numpy() == FILL).all(), "the scratch was written beyond bsmi_blosc_dev_u8_scratch_bytes"
    out = []
    for i, g in enumerate(grid):
        assert 16 < sz[i] <= cb + 16 <= slot, (g, sz[i])
        assert (fr[i, sz[i]:] == FILL).all(), (g, "the slot was written beyond the frame's reported size")
        frame = fr[i, :sz[i]].tobytes()
        want = _expected(host, g, chunk).tobytes()
        ref = _ref_frame(want)
        if frame != ref:      # say where, then let the reader say which of the two is off the format
            at = next((k for k, (a, b) in enumerate(zip(frame, ref)) if a != b), min(len(frame), len(ref)))
            verdict = []
            for name, f in (("device", frame), ("restatement", ref)):
                try:
                    verdict.append(f"{name} frame: strict reader {'reads the chunk' if U.frame_u8_strict(f)[0] == want else 'reads other bytes'}")
                except R.FormatError as e:
                    verdict.append(f"{name} frame: {e}")
            pytest.fail(f"chunk {g}: device frame ({len(frame)} bytes) and restatement ({len(ref)}) differ from byte {at}; " + "; ".join(verdict))
        assert U.frame_u8_strict(frame)[0] == want, g
        for shuffle in (1, 2):
            assert codecs.decode(_lib.Codec(_lib.CODEC_BLOSC, 5, _lib.BLOSC_LZ4, shuffle, 1, 0), frame, cb).tobytes() == want, g
        out.append((g, frame))
    return out


def _affinity_like(shape, seed):
    """the fixture's recipe on another shape: saturating inside objects, dropping at boundaries, the channels alike"""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    g = gaussian_filter(rng.standard_normal(shape[1:]), (1, 4, 4))
    g = g / g.std()
    x = 40 * (np.abs(g) - 0.3)[None] + 2.0 * rng.standard_normal(shape)
    return np.floor(255.0 / (1.0 + np.exp(-x))).astype(np.uint8)


def _kinds(frame):
    """(blocks, blocks kept verbatim, matches at offset 1, matches at other offsets) of a frame that is not stored"""
    blocks = U.frame_blocks(frame)
    seqs = [s for _, sq in blocks if sq for s in sq]
    return len(blocks), sum(sq is None for _, sq in blocks), sum(s[2] == 1 for s in seqs), sum(s[2] > 1 for s in seqs)


# ------------------------------------------------------------------------------------------------ chunk shapes
def test_one_block_chunk():
    (_, frame), = _checked(_affinity_like((2, 4, 64, 64), 21), (2, 4, 64, 64))
    nb, verbatim, runs, far = _kinds(frame)
    assert nb == 1 and not verbatim and runs > 10 and far > 100     # both kinds of candidates won somewhere


def test_a_block_and_a_short_one():
    (_, frame), = _checked(_affinity_like((6, 2, 48, 80), 22), (6, 2, 48, 80))
    blocks = U.frame_blocks(frame)
    assert [n for n, _ in blocks] == [32768, 6 * 2 * 48 * 80 - 32768] and all(sq for _, sq in blocks)
    assert any(s[2] > 1 for s in blocks[1][1])


def test_a_chunk_of_105_bytes():
    host = np.zeros((3, 1, 5, 7), np.uint8)
    host[1] = 200
    (_, frame), = _checked(host, (3, 1, 5, 7))
    (n, seqs), = U.frame_blocks(frame)
    assert n == 105 and seqs == [(1, 34, 1), (36, 34, 1), (71, 29, 1)]     # the last run is cut at n - 5
    noise = np.random.default_rng(23).integers(0, 256, size=(3, 1, 5, 7), dtype=np.uint8)
    (_, frame), = _checked(noise, (3, 1, 5, 7))
    assert U.frame_u8_strict(frame)[1]["stored"] and len(frame) == 121


def test_four_blocks_fixture_b_as_a_chunk():
    (_, frame), = _checked(U.fixture_b()[None], (1, 8, 128, 128))
    nb, verbatim, runs, far = _kinds(frame)
    assert nb == 4 and not verbatim and far > 1000
    assert len(frame) == 16 + 4 * 4 + 4 * 4 + 79539     # the size the CPU test prints for B


# ------------------------------------------------------------------------------------------------ the shared byte cases
@pytest.mark.parametrize("name", ["zeros", "const255", "noise", "A", "bitmap", "far_and_near", "tie", "period3", "period300", "period5000", "end14", "end13",
                                  "end12", *[f"{w}{k}" for k in (1, 4, 11, 12, 13, 17, 300) for w in ("only", "last")]])
def test_byte_cases(name):
    data = _cases()[name]
    (_, frame), = _checked(data.reshape(1, 1, 1, -1), (1, 1, 1, data.size))
    _, info = U.frame_u8_strict(frame)
    # the edge each case is named for (the CPU test holds the restatement to the same)
    if name == "noise" or (name.startswith("only") and name != "only300"):
        assert info["stored"]
        return
    blocks = U.frame_blocks(frame)
    seqs = blocks[0][1]
    if name in ("zeros", "const255"):
        assert all(sq == [(1, n - 6, 1)] for n, sq in blocks) and blocks[-1][0] < U.BLOCK
    elif name == "far_and_near":
        assert [s for s in seqs if s[0] == 1600][0][2] == 300 and not [s for s in seqs if s[2] == 100]
    elif name == "tie":
        assert (1124, 68, 101) in seqs and (1192, 32, 1) in seqs
    elif name == "period5000":
        assert sum(a[1] == b[1] == 68 and a[2] == b[2] == 5000 and a[0] + 68 == b[0] for a, b in zip(seqs, seqs[1:])) >= 20
    elif name == "period3":      # nothing inside the first group of 256, then the table's last position of the group before
        assert seqs[0] == (256, 68, 3) and all(s[2] % 3 == 0 for s in seqs) and len(frame) < data.size // 8
    elif name == "period300":
        assert seqs[0] == (300, 68, 300) and all(s[2] % 300 == 0 for s in seqs) and len(frame) < data.size // 8
    elif name == "end14":
        assert seqs[-1] == (4096 - 13, 8, 1)
    elif name == "end13":
        assert seqs[-1] == (4096 - 12, 7, 1)
    elif name == "end12":
        assert seqs[-1][0] < 4096 - 12
    elif name.startswith("last"):
        k = int(name[4:])
        assert blocks[1] == (k, [(1, k - 6, 1)] if k >= 13 else None)
    elif name == "only300":
        assert blocks == [(300, [(1, 294, 1)])]
    elif name == "bitmap":
        assert not info["stored"] and all(sq for _, sq in blocks)
    else:
        assert name == "A" and len(blocks) == 4


# ------------------------------------------------------------------------------------------------ geometry
def test_overhanging_extents():
    """an array (6, 3, 81, 130) in chunks of (6, 2, 48, 80): the last chunk holds (6, 1, 33, 50) of it, the rest is fill"""
    host = _affinity_like((6, 3, 81, 130), 24)
    res = _checked(host, (6, 2, 48, 80))
    assert len(res) == 8
    g, frame = res[-1]
    assert g == (0, 2, 48, 80)
    want = np.frombuffer(U.frame_u8_strict(frame)[0], np.uint8).reshape(6, 2, 48, 80)
    assert want[:, :1, :33, :50].any() and not want[:, 1:].any() and not want[:, :, 33:].any() and not want[:, :, :, 50:].any()


def test_strided_source_and_chunk_counts():
    """a view into a larger tensor (none of the outer strides is that of the view's shape), cut into 1, 7 and 9 chunks"""
    big = torch.from_numpy(_affinity_like((4, 9, 40, 100), 25)).cuda()
    for sl, chunk, count in (((slice(1, 3), slice(2, 7), slice(3, 35), slice(10, 74)), (2, 5, 32, 64), 1),
                             ((slice(0, 3), slice(1, 8), slice(4, 36), slice(5, 69)), (3, 1, 32, 64), 7),
                             ((slice(1, 4), slice(0, 9), slice(0, 40), slice(20, 100)), (3, 3, 16, 80), 9)):
        view = big[sl]
        assert not view.is_contiguous() and view.stride(3) == 1
        res = _checked(view.cpu().numpy(), chunk, src=view)
        assert len(res) == count


def test_more_chunks_than_one_geometry_launch_carries():
    host = _affinity_like((1, 35, 8, 64), 26)
    res = _checked(host, (1, 1, 8, 64))
    assert len(res) == 35 and len({f for _, f in res}) == 35


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from bootstrapper_amd import _lib
    chunk = (2, 4, 64, 64)
    cb = int(np.prod(chunk))
    src = torch.zeros(chunk, dtype=torch.uint8, device="cuda")
    slot, ns, scratch, frames, sizes = _buffers(1, cb)
    good = dict(src=src, strides=list(src.stride()[:3]), n=1, origins=[0, 0, 0, 0], extents=list(chunk), chunk=chunk, scratch=scratch, ns=ns, frames=frames,
                slot=slot, sizes=sizes)
    assert _call(**good) == 0
    bad = [dict(src=None), dict(strides=None), dict(origins=None), dict(extents=None), dict(chunk=None), dict(scratch=None), dict(frames=None),
           dict(sizes=None), dict(n=0), dict(origins=[0, -1, 0, 0]), dict(extents=[2, 4, 64, 65]), dict(extents=[3, 4, 64, 64]),
           dict(extents=[2, 0, 64, 64]), dict(chunk=(2, 4, 0, 64)), dict(slot=slot - 1), dict(ns=ns - 1),
           dict(chunk=(1, 1025, 128, 256), extents=[1, 1, 1, 1], slot=1 << 40, ns=1 << 40)]
    for change in bad:
        assert _call(**{**good, **change}) == _lib.ERR_INVALID, change
    torch.cuda.synchronize()
    # ... and 1024 blocks exactly are taken (bounds only: the buffers of such a chunk are not allocated here)
    assert int(_lib.lib.bsmi_blosc_dev_u8_frame_bound(1024 * 32768)) == 1024 * 32768 + 16 + 8 * 1024 + 64
    assert int(_lib.lib.bsmi_blosc_dev_u8_frame_bound(105)) == 105 + 16 + 8 + 64


# ------------------------------------------------------------------------------------------------ bs predict
def _predict_setup(tmp_path, golden_dir):
    from bootstrapper_amd.zarr_io import prepare_ds
    d = np.load(os.path.join(golden_dir, "unet_affs_f4i2.npz"))
    sd = {k[2:]: d[k] for k in d.files if k.startswith("w:")}
    setup = tmp_path / "setup_01"
    setup.mkdir()
    nc = {"in_channels": 1, "num_fmaps": 4, "fmap_inc_factor": 2, "downsample_factors": [[1, 2, 2]] * 3,
          "kernel_size_down": [[[3, 3, 3], [3, 3, 3]]] * 4, "kernel_size_up": [[[3, 3, 3], [3, 3, 3]]] * 3,
          "input_shape": [30, 108, 108], "output_shape": [2, 16, 16], "shape_increase": [8, 16, 16],
          "inputs": {"raw": {"dims": 1}}, "outputs": {"3d_affs": {"dtype": "uint8", "dims": 6}}}
    (setup / "net_config.json").write_text(json.dumps(nc))
    ckpt = str(setup / "model_checkpoint_1000")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in sd.items()}}, ckpt + ".ckpt")
    raw = np.random.default_rng(3).integers(0, 256, size=(23, 50, 61), dtype=np.uint8)
    store = str(tmp_path / "vol.zarr")
    ds = prepare_ds(store + "/raw", raw.shape, offset=(80, 8, 8), voxel_size=(40, 4, 4), chunk_shape=(8, 32, 32),
                    dtype=np.uint8, axis_names=["z", "y", "x"], units=["nm"] * 3)
    ds[:] = raw
    cfg = tmp_path / "pred.toml"
    cfg.write_text(f'["01-3d_affs"]\nsetup_dir = "{setup}"\ninput_datasets = ["{store}/raw"]\ncheckpoint = "{ckpt}"\n'
                   f'output_datasets_prefix = "{store}/predictions"\nchain_str = ""\nnum_workers = 1\nnum_gpus = 1\n')
    return store, str(cfg)


def _run(cfg_file, store, name, monkeypatch, switch, prepare, **roi):
    """one `predict_blocks` into <store>/<name>/...; -> (dataset, calls of the device encoder)"""
    from bootstrapper_amd import _lib
    from bootstrapper_amd.predict import get_pred_config, predict_blocks
    from bootstrapper_amd.zarr_io import open_ds
    monkeypatch.delenv("BSMI_DEVICE_FRAMES", raising=False)
    monkeypatch.setenv("BSMI_PRED_DEVICE_FRAMES", switch)
    cfg = get_pred_config(cfg_file, "01-3d_affs", output_datasets_prefix=f"{store}/{name}", **roi)
    prepare(cfg, open_ds(cfg["input_datasets"][0]))
    calls = []
    real = _lib.lib.bsmi_blosc_encode_dev_u8

    def counted(*args):
        calls.append(int(args[3]))
        return real(*args)
    monkeypatch.setattr(_lib.lib, "bsmi_blosc_encode_dev_u8", counted)
    t0 = time.perf_counter()
    state = predict_blocks(cfg, precision="f32")
    monkeypatch.setattr(_lib.lib, "bsmi_blosc_encode_dev_u8", real)
    print(f"predict_blocks into {name}: {time.perf_counter() - t0:.2f} s, {len(calls)} calls of the device encoder")
    assert state.failed_count == 0 and state.completed_count == 3 * 2 * 2
    return open_ds(cfg["output_datasets"][0]), calls


@pytest.fixture(scope="module")
def predicted(tmp_path_factory, golden_dir):
    """the store, its config and the host-path prediction every case is compared with"""
    from bootstrapper_amd.predict import prepare_outputs
    tmp = tmp_path_factory.mktemp("pred_u8")
    store, cfg = _predict_setup(tmp, golden_dir)
    mp = pytest.MonkeyPatch()
    try:
        ds, calls = _run(cfg, store, "host", mp, "0", prepare_outputs)
    finally:
        mp.undo()
    assert not calls
    return store, cfg, ds[:]


def test_predict_writes_device_frames(predicted, monkeypatch):
    from bootstrapper_amd.predict import prepare_outputs
    store, cfg, want = predicted
    ds, calls = _run(cfg, store, "device", monkeypatch, "1", prepare_outputs)
    assert ds.chunks == (6, 10, 32, 32) and ds.shape == (6, 23, 50, 61)      # blocks at the end overhang on all three axes
    assert calls == [1] * 12                                                  # one call per block and dataset, one chunk each
    files = sorted(f for f in os.listdir(ds.path) if not f.startswith(".z"))
    assert files == sorted(f"0.{z}.{y}.{x}" for z in range(3) for y in range(2) for x in range(2))
    for f in files:
        with open(os.path.join(ds.path, f), "rb") as fh:
            data, info = U.frame_u8_strict(fh.read())
        assert info["typesize"] == 1 and info["nbytes"] == 6 * 10 * 32 * 32 and info["blocksize"] == 32768
    assert np.array_equal(ds[:], want)
    with open(os.path.join(ds.path, "0.2.1.1"), "rb") as fh:                  # the corner chunk: fill beyond the dataset's end
        corner = np.frombuffer(U.frame_u8_strict(fh.read())[0], np.uint8).reshape(6, 10, 32, 32)
    assert corner[:, :3, :18, :29].any() and not corner[:, 3:].any() and not corner[:, :, 18:].any() and not corner[:, :, :, 29:].any()


@pytest.mark.parametrize("case", ["zstd", "nested", "off_grid"])
def test_predict_host_path_where_the_gate_says_so(predicted, monkeypatch, case):
    """a zstd store, chunk files in nested directories and a ROI that ends off the chunk grid (inside the dataset) go through the
    host with the switch on"""
    from bootstrapper_amd.predict import prepare_outputs
    from bootstrapper_amd.zarr_io import prepare_ds
    store, cfg, want = predicted

    def prepare(c, in_ds):
        if case == "nested":
            for ds in prepare_outputs(c, in_ds):
                meta = json.load(open(os.path.join(ds.path, ".zarray")))
                meta["dimension_separator"] = "/"
                json.dump(meta, open(os.path.join(ds.path, ".zarray"), "w"))
            return
        # (the driver's own datasets end with the ROI; this one is made the way a caller of the worker script makes them: the whole
        # volume, of which the ROI leaves the last 5 columns out)
        prepare_ds(c["output_datasets"][0], shape=(6, 23, 50, 61), offset=c["output_roi"][0], voxel_size=c["voxel_size"],
                   axis_names=["c^", "z", "y", "x"], units=["nm"] * 3, chunk_shape=(6, 10, 32, 32), dtype=np.uint8,
                   compressor="zstd" if case == "zstd" else "default")
    roi = dict(roi_offset="80 8 8", roi_shape=f"{23 * 40} {50 * 4} {56 * 4}") if case == "off_grid" else {}
    ds, calls = _run(cfg, store, case, monkeypatch, "1", prepare, **roi)
    if case == "off_grid":      # the blocks at x = 0 end on the grid, those at x = 32 end at 56: neither a chunk's end nor the dataset's
        assert calls == [1] * 6
        want = want.copy()
        want[..., 56:] = 0
    else:
        assert not calls
    assert np.array_equal(ds[:], want)
