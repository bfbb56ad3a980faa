"""csrc/blosc_dev.hip at its edges: every frame that `bsmi_blosc_encode_dev_u64` makes here is byte-equal to the sequential
restatement of its rule (tests/blosc_ref.py `encode_frame_ref`), is read back by a reader that enforces the Blosc-1 and LZ4 block
formats and by the host codec, and leaves every byte beyond the sizes that `bsmi_blosc_dev_frame_bound` / `_scratch_bytes`
promise untouched.  The cases are built for: the values at which LZ4's length fields change shape (15, 15 + 255, 15 + 510), runs
that meet the borders of the kernel's 128-byte thread segments, the last 12 bytes of a plane, the thresholds plane -> verbatim
and frame -> stored, chunk shapes that are no powers of two, arrays that overhang the chunk grid, the padded grid, strided
sources, every refusal, and `_LayerWriter` with and without the device path.  Every case asserts from the decoded traces or from
its own positions that it did reach the edge it was built for.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import blosc_ref as R

pytestmark = pytest.mark.gpu

PAD = 4096      # bytes allocated beyond what the size functions promise, per slot and behind the scratch
FILL = 0xA5
N = R.PLANE


def _buffers(n, chunk_bytes, slot=None, scratch=None):
    from bootstrapper_amd import _lib
    slot = int(_lib.lib.bsmi_blosc_dev_frame_bound(chunk_bytes)) if slot is None else slot
    ns = int(_lib.lib.bsmi_blosc_dev_scratch_bytes(n, chunk_bytes)) if scratch is None else scratch
    return (slot, ns, torch.full((ns + PAD,), FILL, dtype=torch.uint8, device="cuda"),
            torch.full((n * (slot + PAD),), FILL, dtype=torch.uint8, device="cuda"),
            torch.full((max(n, 1) * 4,), FILL, dtype=torch.uint8, device="cuda"))


def _call(src, sz, sy, n, origins, extents, chunk, scratch, ns, frames, slot, sizes):
    from bootstrapper_amd import _lib
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)
    return _lib.lib.bsmi_blosc_encode_dev_u64(0, ptr(src), sz, sy, n, (C.c_int64 * len(origins))(*origins) if origins is not None else None,
                                              (C.c_int64 * len(extents))(*extents) if extents is not None else None,
                                              (C.c_int64 * 3)(*chunk) if chunk is not None else None, ptr(scratch), ns, ptr(frames), slot, ptr(sizes),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _expected(host, g, chunk):
    out = np.zeros(chunk, np.uint64)
    part = host[tuple(slice(o, min(o + c, s)) for o, c, s in zip(g, chunk, host.shape))]
    out[:part.shape[0], :part.shape[1], :part.shape[2]] = part
    return out


def _checked(host, chunk, src=None):
    """encode every chunk of the uint64 array `host` (from the device tensor `src`, by default a contiguous copy of it) into
    sentinel-filled slots and scratch; hold every frame against the restatement, the strict reader and the host codec, and every
    byte beyond the promised sizes against the sentinel -> [(grid index, frame, info of the strict reader)]"""
    from bootstrapper_amd import _lib, codecs
    if src is None:
        src = torch.from_numpy(np.ascontiguousarray(host).view(np.int64)).cuda()
    assert tuple(src.shape) == host.shape and src.stride(2) == 1
    grid = [(z, y, x) for z in range(0, host.shape[0], chunk[0]) for y in range(0, host.shape[1], chunk[1]) for x in range(0, host.shape[2], chunk[2])]
    n, cb = len(grid), int(np.prod(chunk)) * 8
    slot, ns, scratch, frames, sizes = _buffers(n, cb)
    _lib.check(_call(src, src.stride(0), src.stride(1), n, [v for g in grid for v in g],
                     [min(c, s - o) for g in grid for o, c, s in zip(g, chunk, host.shape)], chunk, scratch, ns, frames, slot + PAD, sizes))
    torch.cuda.synchronize()
    sz = sizes.cpu().numpy().view(np.uint32)
    fr = frames.cpu().numpy().reshape(n, slot + PAD)
    assert (scratch[ns:].cpu().numpy() == FILL).all(), "the scratch was written beyond bsmi_blosc_dev_scratch_bytes"
    codec = _lib.Codec(_lib.CODEC_BLOSC, 5, _lib.BLOSC_LZ4, 1, 8, 0)
    out = []
    for i, g in enumerate(grid):
        assert 16 < sz[i] <= cb + 16 <= slot, (g, sz[i])
        assert (fr[i, sz[i]:] == FILL).all(), (g, "the slot was written beyond the frame's reported size")
        frame = fr[i, :sz[i]].tobytes()
        want = _expected(host, g, chunk)
        ref = R.encode_frame_ref(want)
        if frame != ref:      # say where, then let the readers say which of the two is off the format
            at = next((k for k, (a, b) in enumerate(zip(frame, ref)) if a != b), min(len(frame), len(ref)))
            verdict = []
            for name, f in (("device", frame), ("restatement", ref)):
                try:
                    verdict.append(f"{name} frame: strict reader {'reads the chunk' if R.blosc1_frame_strict(f)[0] == want.tobytes() else 'reads other bytes'}")
                except R.FormatError as e:
                    verdict.append(f"{name} frame: {e}")
            pytest.fail(f"chunk {g}: device frame ({len(frame)} bytes) and restatement ({len(ref)}) differ from byte {at}; " + "; ".join(verdict))
        data, info = R.blosc1_frame_strict(frame)
        assert data == want.tobytes(), g
        assert codecs.decode(codec, frame, cb).tobytes() == want.tobytes(), g
        out.append((g, frame, info))
    return out


def _traces(results):
    """[(literal count, match length)] of every sequence of every lz4 plane of the frames"""
    return [t for _, _, info in results for blk in info["traces"] for tr in blk if tr for t in tr]


def _one_block(planes):
    assert len(planes) == 8
    return R.planes_to_u64(planes).reshape(8, 64, 64)


def _other(*avoid):
    """a byte value that is none of `avoid`"""
    return next(v for v in (0x11, 0x22, 0x33, 0x44) if v not in [int(a) for a in avoid])


def _labels(rng, shape, run):
    """label volume: ids above 2^32 in runs of about `run` voxels along x, 2 % of the voxels background"""
    z, y, x = shape
    ids = rng.integers(1 << 32, 1 << 38, size=(z, y, x // run + 2), dtype=np.uint64)
    rep = np.repeat(ids, run, axis=2)[:, :, :x]
    rep[rng.random(shape) < 0.02] = 0
    return np.ascontiguousarray(rep)


# ------------------------------------------------------------------------------------------------ a. length sweep
STRETCHES = [0, 1, 2, 13, 14, 15, 16, 17, 268, 269, 270, 271, 272, 523, 524, 525, 526]
RUNS = [1, 2, 7, 8, 9, 18, 19, 20, 21, 22, 127, 128, 129, 255, 256, 257, 273, 274, 275, 276, 277, 400, 528, 529, 530, 531]


def _sweep_plane(rng):
    """stretches in which no byte equals the one before it, alternating with runs, lengths drawn from the two lists"""
    out = np.zeros(0, np.uint8)
    prev = 0
    while out.size < N:
        st = R.distinct_bytes(rng, int(rng.choice(STRETCHES)), avoid=prev)
        prev = int(st[-1]) if st.size else prev
        v = (prev + int(rng.integers(1, 256))) % 256
        out = np.concatenate([out, st, np.full(int(rng.choice(RUNS)), v, np.uint8)])
        prev = v
    return out[:N]


def test_length_fields_at_15_270_and_525():
    rng = np.random.default_rng(1)
    chunks = [_one_block([_sweep_plane(rng) for _ in range(8)]) for _ in range(2)]
    tr = _traces(_checked(np.concatenate(chunks), (8, 64, 64)))
    lits = {lit for lit, ml in tr if ml}
    m4 = {ml - 4 for _, ml in tr if ml}
    print("literal counts", sorted(lits), "match lengths - 4", sorted(m4))
    assert lits >= {1, 14, 15, 16, 269, 270, 271, 524, 525, 526}, sorted(lits)
    assert m4 >= {3, 14, 15, 16, 269, 270, 271, 524, 525, 526}, sorted(m4)


# ------------------------------------------------------------------------------------------------ b. segment hand-over
def _handover_planes(rng):
    """non-repeating planes with single runs 1024 bytes apart: starts 128 k + d for d = -9 .. 1, k = 1 and 2, all of 7 lengths"""
    cases = [(d, ln, k) for d in range(-9, 2) for k in (1, 2) for ln in (7, 8, 9, 128, 129, 300, 700)]    # every plane gets long runs
    planes, runs = [], []
    for at in range(0, len(cases), 32):
        p = R.distinct_bytes(rng, N)
        for j, (d, ln, k) in enumerate(cases[at:at + 32]):
            s = 1024 * j + 128 * k + d
            assert 1024 * j < s and s + ln < 1024 * (j + 1) and s + ln < N - 12
            p[s:s + ln] = _other(p[s - 1], p[s + ln])
            runs.append((s, ln))
        planes.append(p)
    return planes + [R.distinct_bytes(rng, N) for _ in range(8 - len(planes))], runs


def test_runs_across_the_borders_of_the_thread_segments():
    rng = np.random.default_rng(2)
    planes, runs = _handover_planes(rng)
    assert len(planes) == 8 and len(runs) == 2 * 7 * 11
    assert {(d, ln) for d in range(-9, 2) for ln in (7, 8, 9, 128, 129, 300, 700)} == {((s + 9) % 128 - 9, ln) for s, ln in runs}
    long = [(s, ln) for s, ln in runs if ln >= 8]
    assert any(s % 128 == 127 for s, _ in long) and any(s % 128 == 0 for s, _ in long)      # starts on a segment's last / first byte
    assert any((s + ln) % 128 == 0 for s, ln in long)                                         # ends exactly at a segment's end
    assert any((s + 7) % 128 == 0 for s, _ in long)                                           # the eighth byte opens the next segment
    assert any((s + ln) // 128 - (s // 128 + 1) >= 3 for s, ln in long)                      # three whole segments without a start
    assert any(ln == 7 and (s + 6) // 128 != s // 128 for s, ln in runs)                      # a run of 7 over a border stays literals
    res = _checked(_one_block(planes), (8, 64, 64))
    # every long run came out as one match of its length - 1, and no run of 7 became one
    want = sorted(ln - 1 for _, ln in long)
    assert sorted(ml for _, ml in _traces(res) if ml) == want


# ------------------------------------------------------------------------------------------------ c. tail
def _tail_plane(rng, cut, run=40):
    """non-repeating bytes, a run over [1000, 3000) that makes LZ4 worth it, and a run of `run` bytes that ends at n - cut"""
    p = R.distinct_bytes(rng, N)
    p[1000:3000] = _other(p[999], p[3000])
    end = N - cut
    p[end - run:end] = _other(p[end - run - 1], p[end] if cut else 0)
    return p


def test_the_last_twelve_bytes_stay_literals():
    """a 40-byte run that ends 0 .. 20 bytes before the plane's end, with non-repeating bytes behind it (the planes carry one more
    run near their start: a single run of 40 gains less than the closing literals' length bytes cost, and the plane would be kept
    verbatim), runs of 8 around the limit, and planes that are one run"""
    rng = np.random.default_rng(3)
    planes = [_tail_plane(rng, cut) for cut in range(21)]
    planes += [_tail_plane(rng, cut, run=8) for cut in (11, 12, 13, 14)]
    constant = np.full(N, 0x5A, np.uint8)
    but_tail = np.concatenate([np.full(N - 12, 0x5A, np.uint8), R.distinct_bytes(rng, 12, avoid=0x5A)])
    from_zero = R.distinct_bytes(rng, N)
    from_zero[:300] = _other(from_zero[300])
    late = R.distinct_bytes(rng, N)
    late[20000:20400] = _other(late[19999], late[20400])
    planes += [constant, but_tail, from_zero, late] + [np.zeros(N, np.uint8)] * 3
    assert len(planes) == 32
    res = _checked(np.concatenate([_one_block(planes[i:i + 8]) for i in range(0, 32, 8)]), (8, 64, 64))
    tr = [t for _, _, info in res for t in info["traces"][0]]
    for cut in range(21):      # the 40-byte run that ends `cut` bytes before the plane's end: cut back to n - 12 where it reaches beyond
        kept = 40 - max(0, 12 - cut)
        assert tr[cut] == [(1001, 1999), (N - cut - 40 - 3000 + 1, kept - 1), (max(12, cut), 0)], (cut, tr[cut])
    # runs of 8 around the limit: 11 -> 7 bytes are left, literals; 12 ends exactly at n - 12; 13 and 14 end short of it
    assert tr[21] == [(1001, 1999), (N - 3000, 0)]
    assert [t[1:] for t in tr[22:25]] == [[(N - cut - 8 - 3000 + 1, 7), (cut, 0)] for cut in (12, 13, 14)]
    assert tr[25] == tr[26] == [(1, N - 13), (12, 0)]          # one match: 128 extension bytes of 255 and one of 96
    assert tr[27] == [(1, 299), (N - 300, 0)]
    assert tr[28] == [(20001, 399), (N - 20400, 0)]


# ------------------------------------------------------------------------------------------------ d. verbatim and stored thresholds
def _plane_with_stream_of(rng, target):
    """a non-repeating plane with a few runs of 8 to 12 and one run tuned so that its restated LZ4 block has `target` bytes"""
    p = R.distinct_bytes(rng, N)
    for k, ln in enumerate((8, 9, 10, 11, 12)):
        s = 20000 + 500 * k
        p[s:s + ln] = _other(p[s - 1], p[s + ln])
    for ln in range(8, 600):
        q = p.copy()
        q[1000:1000 + ln] = _other(q[999], q[1000 + ln])
        if len(R.plane_stream_ref(q)) == target:
            return q
    raise AssertionError(f"no run length gives a stream of {target} bytes")


def test_verbatim_planes_and_stored_frames_at_the_documented_sizes():
    rng = np.random.default_rng(4)
    noise = [R.distinct_bytes(rng, N) for _ in range(7)]
    chunks = []
    for target in (N - 1, N, N + 1):                 # one byte shorter than the plane: lz4; as long or longer: verbatim
        chunks.append(_one_block([_plane_with_stream_of(rng, target)] + [np.zeros(N, np.uint8)] * 7))
    # one block, 7 planes verbatim: cbytes = 16 + 4 + 7 * (4 + 32768) + 4 + the eighth plane's stream
    for cbytes in (R.BLOCK + 15, R.BLOCK + 16, R.BLOCK + 17):
        chunks.append(_one_block(noise[:3] + [_plane_with_stream_of(rng, cbytes - 20 - 7 * (4 + N) - 4)] + noise[3:]))
    res = _checked(np.concatenate(chunks), (8, 64, 64))
    infos = [info for _, _, info in res]
    assert infos[0]["lengths"][0][0] == N - 1 and infos[0]["traces"][0][0] is not None
    assert infos[1]["lengths"][0][0] == N and infos[1]["traces"][0][0] is None
    assert infos[2]["lengths"][0][0] == N and infos[2]["traces"][0][0] is None
    assert not infos[3]["stored"] and infos[3]["cbytes"] == R.BLOCK + 15 and infos[3]["flags"] == 0x21
    assert [ln == N for ln in infos[3]["lengths"][0]] == [True] * 3 + [False] + [True] * 4
    for info in infos[4:]:                            # nbytes + 16 or more: stored, flag 2, the chunk's own bytes
        assert info["stored"] and info["flags"] == 0x23 and info["cbytes"] == R.BLOCK + 16


# ------------------------------------------------------------------------------------------------ e. geometry
GEOMETRY = [
    # chunk, array, data, blocks in the request; what overhangs
    ((1, 1, 32768), (1, 1, 32767), "labels", 1),       # x by 1
    ((1, 1, 32768), (7, 1, 32768), "labels", 7),
    ((1, 1, 32768), (2, 4, 32765), "noise", 8),        # x by 3, stored
    ((16, 64, 96), (40, 64, 96), "labels", 9),         # z: the last chunk has 8 of 16 sections
    ((16, 64, 96), (16, 64, 95), "labels", 3),         # x by 1: one zero per row
    ((16, 64, 96), (16, 64, 189), "noise", 6),         # x by 3 in the second chunk: stored, 3 zeros per row
    ((3, 128, 256), (3, 128, 249), "labels", 3),       # x by 7: the fill of a row is one byte short of a match
    ((3, 128, 256), (3, 128, 248), "labels", 3),       # x by 8: the fill of a row is the shortest match
    ((3, 128, 256), (3, 100, 256), "labels", 3),       # y
    ((3, 128, 256), (3, 128, 509), "noise", 6),        # x by 3 in the second chunk: stored
    ((2, 3, 16384), (2, 3, 16381), "labels", 3),       # x by 3
    ((2, 3, 16384), (3, 3, 16384), "noise", 6),        # z: the second chunk is half fill
]


@pytest.mark.parametrize("chunk,shape,kind,blocks", GEOMETRY, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_chunk_shapes_that_are_no_powers_of_two_and_arrays_that_overhang(chunk, shape, kind, blocks):
    rng = np.random.default_rng(sum(shape))
    host = _labels(rng, shape, 20) if kind == "labels" else rng.integers(1, 1 << 63, size=shape, dtype=np.uint64) | np.uint64(0x0101010101010101)
    res = _checked(host, chunk)
    nb = int(np.prod(chunk)) * 8 // R.BLOCK
    assert len(res) * nb == blocks
    fills = 0
    for g, frame, info in res:
        over = [o + c > s for o, c, s in zip(g, chunk, shape)]
        # noise with at most 3 voxels of fill per row has nothing to gain and is stored; half a chunk of fill, or labels, is not
        assert info["stored"] == (kind == "noise" and not over[0]), g
        if info["stored"] and over[2]:          # the stored path's own gather put the fill where the array ends
            back = np.frombuffer(frame[16:], np.uint64).reshape(chunk)
            assert (back[:, :, shape[2] - g[2]:] == 0).all() and (back[:, :, :shape[2] - g[2]] != 0).all(), g
            fills += 1
    assert fills or kind == "labels" or shape[2] % chunk[2] == 0


def test_a_source_with_row_and_section_strides():
    """rows further apart than a row of chunks is long, sections no whole number of rows apart"""
    rng = np.random.default_rng(5)
    shape, chunk = (11, 70, 128), (8, 64, 64)
    sy = 2 * 64 + 5
    sz = 70 * sy + 3
    assert sy > chunk[2] * 2 and sz % sy
    flat = rng.integers(1 << 32, 1 << 40, size=shape[0] * sz, dtype=np.uint64)
    flat = np.repeat(flat[::16], 16)[:flat.size]                       # runs of 16 across the rows' gaps too
    host = np.lib.stride_tricks.as_strided(flat, shape, (sz * 8, sy * 8, 8))
    src = torch.as_strided(torch.from_numpy(flat.view(np.int64)).cuda(), shape, (sz, sy, 1))
    res = _checked(np.ascontiguousarray(host), chunk, src=src)
    assert len(res) == 8 and not any(info["stored"] for _, _, info in res)


# ------------------------------------------------------------------------------------------------ third-party readers
@pytest.fixture(scope="module")
def edge_frames():
    """frames of a sweep chunk, the hand-over chunk, a chunk of tails and a stored one -> [(chunk, frame, info)]"""
    rng = np.random.default_rng(6)
    chunks = [_one_block([_sweep_plane(rng) for _ in range(8)]), _one_block(_handover_planes(rng)[0]),
              _one_block([_tail_plane(rng, cut) for cut in (0, 1, 5, 11, 12, 13)] + [np.full(N, 9, np.uint8), R.distinct_bytes(rng, N)]),
              rng.integers(0, 1 << 63, size=(8, 64, 64), dtype=np.uint64)]
    host = np.concatenate(chunks)
    return [(_expected(host, g, (8, 64, 64)), frame, info) for g, frame, info in _checked(host, (8, 64, 64))]


def test_c_blosc_reads_the_device_frames(edge_frames):
    blosc = R.find_c_blosc()
    if blosc is None:
        pytest.skip("c-blosc is not installed on this machine")
    assert [info["stored"] for _, _, info in edge_frames] == [False, False, False, True]
    for i, (want, frame, _) in enumerate(edge_frames):
        assert R.c_blosc_decode(blosc, frame, want.nbytes) == want.tobytes(), i


def test_liblz4_reads_the_planes_of_the_device_frames(edge_frames):
    lz4 = R.find_lz4()
    if lz4 is None:
        pytest.skip("liblz4 is not installed on this machine")
    seen = 0
    for i, (want, frame, info) in enumerate(edge_frames[:3]):
        at = info["starts"][0]
        for p, (ln, tr) in enumerate(zip(info["lengths"][0], info["traces"][0])):
            if tr is not None:
                assert R.liblz4_decode(lz4, frame[at + 4:at + 4 + ln], N) == want.reshape(-1).view(np.uint8)[p::8].tobytes(), (i, p)
                seen += 1
            at += 4 + ln
    assert seen >= 18


# ------------------------------------------------------------------------------------------------ f. refusals
def test_refusals_launch_nothing():
    from bootstrapper_amd import _lib
    chunk = (8, 64, 64)
    cb = R.BLOCK
    src = torch.zeros(chunk, dtype=torch.int64, device="cuda")
    slot, ns, scratch, frames, sizes = _buffers(1, cb)
    ok = dict(src=src, sz=64 * 64, sy=64, n=1, origins=[0, 0, 0], extents=[8, 64, 64], chunk=chunk, scratch=scratch, ns=ns, frames=frames,
              slot=slot, sizes=sizes)
    whole = "device Blosc frames take chunks of whole 256 KiB blocks"
    cases = [
        (dict(chunk=(8, 64, 60), extents=[8, 64, 60]), whole + r".*a chunk of 245760 bytes"),
        (dict(chunk=(1025, 1, 32768), extents=[1, 1, 1]), whole + r".*a chunk of 268697600 bytes"),
        (dict(slot=slot - 1), "scratch or frame slots too small"),
        (dict(ns=ns - 1), "scratch or frame slots too small"),
        (dict(extents=[8, 0, 64]), "chunk 0 has a bad extent"),
        (dict(extents=[8, 64, 65]), "chunk 0 has a bad extent"),
        (dict(extents=[9, 64, 64]), "chunk 0 has a bad extent"),
        (dict(origins=[0, -1, 0]), "chunk 0 has a bad extent"),
        (dict(n=0), "null argument"),
        (dict(n=-1), "null argument"),
    ] + [(dict([(k, None)]), "null argument") for k in ("src", "origins", "extents", "chunk", "scratch", "frames", "sizes")]
    for change, message in cases:
        with pytest.raises(_lib.BsmiError, match=message) as e:
            _lib.check(_call(**dict(ok, **change)))
        assert e.value.code == -1, change                      # BSMI_ERR_INVALID
    torch.cuda.synchronize()
    for t in (scratch, frames, sizes):
        assert (t.cpu().numpy() == FILL).all()
    # the same buffers do take the call that none of the changes was made to
    _lib.check(_call(**ok))
    torch.cuda.synchronize()
    assert int(sizes.cpu().numpy().view(np.uint32)[0]) == len(R.encode_frame_ref(np.zeros(chunk, np.uint64)))


# ------------------------------------------------------------------------------------------------ g. the writer, both ways
def test_layer_writer_with_and_without_device_frames(tmp_path, monkeypatch):
    from bootstrapper_amd.post.watershed import _LayerWriter
    from bootstrapper_amd.zarr_io import open_ds, prepare_ds
    import os
    rng = np.random.default_rng(7)
    host = _labels(rng, (20, 100, 128), 20)
    vol = torch.from_numpy(host.view(np.int64)).cuda()
    paths = {}
    for mode in ("device", "host"):
        if mode == "host":
            monkeypatch.setenv("BSMI_DEVICE_FRAMES", "0")
        else:
            monkeypatch.delenv("BSMI_DEVICE_FRAMES", raising=False)
        ds = prepare_ds(str(tmp_path / f"{mode}.zarr") + "/labels", host.shape, chunk_shape=(8, 64, 64), dtype=np.uint64, voxel_size=(1, 1, 1),
                        offset=(0, 0, 0))
        w = _LayerWriter(torch.device("cuda", 0), 8)
        w.submit(ds, vol, 0, 0)
        w.drain()
        w.close()
        assert bool(w.devbuf) == (mode == "device")
        assert np.array_equal(open_ds(ds.path)[:], host), mode
        paths[mode] = ds
    ds = paths["device"]
    files = sorted(f for f in os.listdir(ds.path) if not f.startswith("."))
    assert len(files) == 3 * 2 * 2
    for name in files:
        g = tuple(int(i) * c for i, c in zip(name.split("."), (8, 64, 64)))
        with open(os.path.join(ds.path, name), "rb") as f:
            frame = f.read()
        want = _expected(host, g, (8, 64, 64))
        assert frame == R.encode_frame_ref(want), name
        assert R.blosc1_frame_strict(frame)[0] == want.tobytes(), name
    # the host path's files are Blosc frames of the same chunks in the host codec's own layout (blocks not split)
    for name in files:
        with open(os.path.join(paths["host"].path, name), "rb") as f:
            data, info = R.blosc1_read_strict(f.read())
        g = tuple(int(i) * c for i, c in zip(name.split("."), (8, 64, 64)))
        assert data == _expected(host, g, (8, 64, 64)).tobytes() and info["flags"] & 16, name
