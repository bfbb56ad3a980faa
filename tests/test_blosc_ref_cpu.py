"""tests/blosc_ref.py on its own, without a GPU: the strict Blosc-1 / LZ4 reader is not stricter than the real writers (it reads
every lz4 frame that c-blosc wrote into tests/golden/codec_cases.npz) and does reject what the formats forbid; the restatement of
csrc/blosc_dev.hip's rule writes frames that the strict reader, the host codec, liblz4 and c-blosc read back; the host codec's own
lz4 encoders (csrc/chunk_codec.cpp `lz4_encode`, as numcodecs-lz4 and inside Blosc) obey LZ4's end-of-block rules; and
`_LayerWriter._device_frames_ok` says no for every reason it has."""
import json
import os

import numpy as np
import pytest

import blosc_ref as R
from bootstrapper_amd import _lib, codecs
from test_codecs import _payloads

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codec_cases.npz")


# ------------------------------------------------------------------------------------------------ the strict reader
def test_strict_reader_reads_every_lz4_frame_that_c_blosc_wrote():
    g = np.load(GOLD)
    seen, split, matches = set(), 0, 0
    for key in g.files:
        part = key.split("__")
        if part[0] != "blosc" or not part[2].startswith("lz4"):
            continue
        frame = g[key].tobytes()
        if frame[2] & 4:          # bit shuffle: not restated
            assert part[3] == "s2", key
            continue
        data, info = R.blosc1_read_strict(frame)
        assert data == g["plain__" + part[1]].tobytes(), key
        seen.add((part[1], part[2], part[3], part[4]))
        split += any(len(ln) > 1 for ln in info["lengths"])
        matches += sum(1 for tr in info["traces"] for t in tr if t for _, ml in t if ml)
    plains = {k[len("plain__"):] for k in g.files if k.startswith("plain__")}
    assert {s[0] for s in seen} == plains and {s[1] for s in seen} == {"lz4", "lz4hc"}
    assert {s[2] for s in seen} >= {"s0", "s1"} and {s[3] for s in seen} == {"b0", "b4096"}
    assert len(seen) >= 4 * len(plains) and split > 0 and matches > 1000   # split and unsplit blocks, and real matches, were read


def _seq(lit, off, ml):
    """one LZ4 sequence with short lengths: literals, offset, match length (ml = 0: closing literals)"""
    assert len(lit) < 15 and (ml == 0 or 4 <= ml < 19)
    return bytes([len(lit) << 4 | (ml - 4 if ml else 0)]) + bytes(lit) + (off.to_bytes(2, "little") if ml else b"")


def test_strict_lz4_accepts_the_limits_and_rejects_what_lies_beyond():
    # at the limits: a match that starts exactly 12 and ends exactly 5 bytes before the end (n = 13: the smallest block with one)
    ok = _seq(b"a", 1, 7) + _seq(b"vwxyz", 0, 0)
    data, trace = R.lz4_block_strict(ok, 13)
    assert data == b"a" * 8 + b"vwxyz" and trace == [(1, 7), (5, 0)]
    assert R.lz4_block_strict(b"\x00", 0) == (b"", [(0, 0)])
    assert R.lz4_block_strict(_seq(b"abc", 0, 0), 3) == (b"abc", [(3, 0)])
    # lengths of 15, 15 + 255 and more in both fields
    lit = bytes(range(1, 255)) + bytes(range(1, 20))
    long = bytes([0xff, 255, len(lit) - 15 - 255]) + lit + b"\x01\x00" + bytes([255, 255, 3]) + _seq(b"0123456789ab", 0, 0)
    data, trace = R.lz4_block_strict(long, len(lit) + 532 + 12)
    assert trace == [(len(lit), 532), (12, 0)] and data == lit + lit[-1:] * 532 + b"0123456789ab"
    bad = {
        "starts at 9, inside the last 12": (_seq(b"abcdefghi", 1, 4) + _seq(b"tuvwxyz", 0, 0), 20),
        "ends at 9, inside the last 5": (_seq(b"a", 1, 8) + _seq(b"wxyz", 0, 0), 13),
        "ends at 30, inside the last 5": (_seq(b"a", 1, 18) + _seq(b"b", 1, 10) + _seq(b"xyz", 0, 0), 32),
        "offset 0": (_seq(b"a", 0, 7) + _seq(b"vwxyz", 0, 0), 13),
        "offset 2 reaches before": (_seq(b"a", 2, 7) + _seq(b"vwxyz", 0, 0), 13),
        "ends after a match": (_seq(b"a", 1, 7), 13),                                   # no closing literals at all ...
        "ends at 13, inside the last 5": (_seq(b"a", 1, 12) + b"\x00", 13),             # ... or an empty closing sequence
        "last token names a match": (_seq(b"a", 1, 7) + b"\x53vwxyz", 13),
        "12 bytes came out": (_seq(b"a", 1, 7) + _seq(b"wxyz", 0, 0), 13),
        "literals run past the 13": (_seq(b"a", 1, 7) + _seq(b"uvwxyz", 0, 0), 13),
        "literals run past the input": (_seq(b"a", 1, 7) + b"\x50vwxy", 13),
        "empty stream": (b"", 0),
    }
    for why, (stream, n) in bad.items():
        with pytest.raises(R.FormatError, match=why):
            R.lz4_block_strict(stream, n)


def _label_chunk(rng, nblocks, run=11):
    ids = rng.integers(1, 1 << 38, size=nblocks * R.PLANE // run + 2, dtype=np.uint64)
    return np.repeat(ids, run)[:nblocks * R.PLANE]


def test_strict_frame_reader_rejects_broken_headers_and_tables():
    rng = np.random.default_rng(2)
    chunk = _label_chunk(rng, 3)
    frame = R.encode_frame_ref(chunk)
    data, info = R.blosc1_frame_strict(frame)
    assert data == chunk.tobytes() and len(info["starts"]) == 3 and not info["stored"]

    def patched(at, value, width=4, base=frame):
        return base[:at] + int(value).to_bytes(width, "little") + base[at + width:]

    s = info["starts"]
    swapped = patched(16 + 4, s[2], base=patched(16 + 8, s[1]))        # blocks 1 and 2 named in each other's place
    stored = R.encode_frame_ref(rng.integers(0, 1 << 63, size=R.PLANE, dtype=np.uint64))
    assert stored[2] == 0x23 and len(stored) == R.BLOCK + 16
    bad = [
        ("cbytes", patched(12, len(frame) + 1)),
        ("cbytes", patched(12, len(frame) - 1)),
        ("cbytes", frame + b"\0"),
        ("do not ascend", swapped),
        ("not right behind the table", patched(16, s[0] + 4)),
        ("the block before it ends", patched(16 + 4, s[1] + 1)),
        ("version bytes 1", patched(0, 1, 1)),
        ("version bytes 2, 2", patched(1, 2, 1)),
        ("flags 0x31", patched(2, 0x31, 1)),                             # "blocks are not split" set: the planes would be one stream
        ("bit shuffle", patched(2, 0x25, 1)),
        ("not lz4", patched(2, 0x81, 1)),
        ("typesize 4", patched(3, 4, 1)),
        ("block size 131072", patched(8, 131072)),
        ("a stored frame of", patched(12, len(stored) + 4, base=stored + b"\0" * 4)),   # cbytes agrees with the length, nbytes does not
    ]
    for why, f in bad:
        with pytest.raises(R.FormatError, match=why):
            R.blosc1_frame_strict(f)
    # a plane whose length prefix is off by one leaves a gap before the next block
    at = s[0]
    with pytest.raises(R.FormatError):
        R.blosc1_frame_strict(patched(at, int.from_bytes(frame[at:at + 4], "little") - 1))


# ------------------------------------------------------------------------------------------------ the restatement
def _ref_chunks():
    rng = np.random.default_rng(7)
    mixed = rng.integers(0, 1 << 16, size=R.PLANE, dtype=np.uint64) | np.uint64(0x0000123400000000)
    tail = _label_chunk(rng, 1, 200)
    tail[-5000:] = 77
    return {"labels": _label_chunk(rng, 2), "labels20": _label_chunk(rng, 1, 20), "mixed": mixed, "tail": tail,
            "zeros": np.zeros(R.PLANE, np.uint64), "noise": rng.integers(0, 1 << 63, size=R.PLANE, dtype=np.uint64)}


@pytest.fixture(scope="module")
def ref_frames():
    return {k: (v, R.encode_frame_ref(v)) for k, v in _ref_chunks().items()}


def test_restated_frames_read_back_through_the_strict_reader_and_the_host_codec(ref_frames):
    codec = _lib.Codec(_lib.CODEC_BLOSC, 5, _lib.BLOSC_LZ4, 1, 8, 0)
    for kind, (chunk, frame) in ref_frames.items():
        data, info = R.blosc1_frame_strict(frame)
        assert data == chunk.tobytes(), kind
        assert codecs.decode(codec, frame, chunk.nbytes).tobytes() == chunk.tobytes(), kind
        assert info["stored"] == (kind == "noise")
        if kind == "mixed":      # noise planes verbatim next to constant ones inside one lz4 frame
            assert info["lengths"][0][:2] == [R.PLANE, R.PLANE] and info["traces"][0][0] is None and info["traces"][0][7] is not None
        if kind == "zeros":      # one match per plane: the token, the literal, the offset, 128 bytes of 255 and one more, 12 + 1 closing
            assert info["traces"][0] == [[(1, R.PLANE - 13), (12, 0)]] * 8 and len(frame) == 16 + 4 + 8 * (4 + 1 + 1 + 2 + 129 + 13)
        if kind == "labels20":   # fragments 20 voxels wide: match length - 4 sits right at 15
            assert {ml - 4 for tr in info["traces"][0] if tr for _, ml in tr if ml} >= {15}


def _splits(frame, info):
    """(offset, length, trace) of every split of a frame that is not stored"""
    for b, start in enumerate(info["starts"]):
        at = start
        for ln, tr in zip(info["lengths"][b], info["traces"][b]):
            yield at + 4, ln, tr
            at += 4 + ln


def test_restated_frames_read_back_through_liblz4(ref_frames):
    lz4 = R.find_lz4()
    if lz4 is None:
        pytest.skip("liblz4 is not installed on this machine")
    planes = 0
    for kind, (chunk, frame) in ref_frames.items():
        data, info = R.blosc1_frame_strict(frame)
        shuffled = np.frombuffer(chunk.tobytes(), np.uint8).reshape(-1, R.PLANE, 8)
        for i, (at, ln, tr) in enumerate(_splits(frame, info)):
            if tr is not None:
                assert R.liblz4_decode(lz4, frame[at:at + ln], R.PLANE) == shuffled[i // 8, :, i % 8].tobytes(), (kind, i)
                planes += 1
    assert planes >= 30


def test_restated_frames_read_back_through_c_blosc(ref_frames):
    blosc = R.find_c_blosc()
    if blosc is None:
        pytest.skip("c-blosc is not installed on this machine")
    for kind, (chunk, frame) in ref_frames.items():
        assert R.c_blosc_decode(blosc, frame, chunk.nbytes) == chunk.tobytes(), kind


def test_restatement_helpers():
    rng = np.random.default_rng(3)
    pats = [rng.integers(0, 256, R.PLANE, dtype=np.uint8) for _ in range(8)]
    u = R.planes_to_u64(pats)
    assert u.dtype == np.uint64 and u.shape == (R.PLANE,)
    by = u.view(np.uint8).reshape(R.PLANE, 8)
    assert all(np.array_equal(by[:, p], pats[p]) for p in range(8))
    d = R.distinct_bytes(rng, 5000, avoid=9)
    assert d[0] != 9 and (d[1:] != d[:-1]).all()
    # a run of 7 stays literals, a run of 8 becomes a match of 7; the plane's last 12 bytes are never part of a match
    for run, want in ((7, [(R.PLANE, 0)]), (8, [(101, 7), (R.PLANE - 108, 0)])):
        p = R.distinct_bytes(rng, R.PLANE)
        p[100:100 + run] = p[100]
        p[100 + run] = p[100] ^ 1
        p[99] = p[100] ^ 2
        assert R.lz4_block_strict(R.plane_stream_ref(p), R.PLANE)[1] == want
    p = R.distinct_bytes(rng, R.PLANE)
    p[-40:] = 5
    p[-41] = 6
    assert R.lz4_block_strict(R.plane_stream_ref(p), R.PLANE)[1] == [(R.PLANE - 39, 27), (12, 0)]
    noise = R.distinct_bytes(rng, R.PLANE).tobytes()
    assert len(R.plane_stream_ref(noise)) == R.PLANE + 1 + 129 and R.encode_plane_ref(noise) == noise    # no gain: verbatim


# ------------------------------------------------------------------------------------------------ the host codec's lz4 encoder
def test_host_lz4_encoders_obey_the_end_of_block_rules():
    matches = 0
    for name, (arr, ts) in _payloads().items():
        plain = arr.tobytes()
        enc = codecs.encode(codecs.from_config({"id": "lz4"}, ts), arr)      # numcodecs lz4: the size, then one block
        assert int.from_bytes(enc[:4], "little") == len(plain), name
        if plain:
            data, trace = R.lz4_block_strict(enc[4:], len(plain))
            assert data == plain, name
            matches += sum(1 for _, ml in trace if ml)
        for shuffle in (0, 1):
            for blocksize in (0, 4096):
                conf = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": shuffle, "blocksize": blocksize}
                frame = codecs.encode(codecs.from_config(conf, ts), arr)
                data, info = R.blosc1_read_strict(frame)
                assert data == plain, (name, conf)
                assert info["typesize"] == ts and info["flags"] & 16, (name, conf)
                matches += sum(1 for tr in info["traces"] for t in tr if t for _, ml in t if ml)
    assert matches > 1000


# ------------------------------------------------------------------------------------------------ the writer's gate
def test_device_frames_ok_truth_table(tmp_path, monkeypatch):
    import torch
    from bootstrapper_amd.post.watershed import _LayerWriter
    from bootstrapper_amd.zarr_io import open_ds, prepare_ds
    monkeypatch.delenv("BSMI_DEVICE_FRAMES", raising=False)
    ok = _LayerWriter._device_frames_ok
    shape, chunks = (20, 100, 128), (8, 64, 64)

    def make(name, compressor="default", chunk_shape=chunks, dtype=np.uint64, fill=None):
        ds = prepare_ds(str(tmp_path / f"{name}.zarr") + "/v", shape, chunk_shape=chunk_shape, dtype=dtype, compressor=compressor,
                        voxel_size=(1, 1, 1), offset=(0, 0, 0))
        if fill is not None:
            with open(os.path.join(ds.path, ".zarray")) as f:
                meta = json.load(f)
            meta["fill_value"] = fill
            with open(os.path.join(ds.path, ".zarray"), "w") as f:
                json.dump(meta, f)
            ds = open_ds(ds.path, "r+")
            assert ds.fill_value == fill
        return ds

    def piece(z=8, y=100, x=128, dtype=torch.int64):
        return torch.zeros((z, y, x), dtype=dtype)

    blosc = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}
    default = make("default")
    assert default.chunk_nbytes == 256 * 1024
    # yes: whole layers of chunks from a chunk boundary on, up to a chunk boundary or the array's end
    assert ok(default, 0, 0, piece())
    assert ok(default, 8, 0, piece())
    assert ok(default, 16, 0, piece(z=4))                    # the last, partial layer: it ends with the array
    assert ok(default, 0, 64, piece(y=36))                   # from a chunk row on to the array's end
    assert ok(default, 0, 0, piece(y=64))                    # ... or up to a chunk row
    assert ok(make("explicit", dict(blosc, blocksize=256 * 1024)), 0, 0, piece())
    # no, one cause at a time
    assert not ok(make("zstd", {"id": "blosc", "cname": "zstd", "clevel": 5, "shuffle": 1, "blocksize": 0}), 0, 0, piece())
    assert not ok(make("zstd_plain", "zstd"), 0, 0, piece())
    assert not ok(make("bitshuffle", dict(blosc, shuffle=2)), 0, 0, piece())
    assert not ok(make("noshuffle", dict(blosc, shuffle=0)), 0, 0, piece())
    assert not ok(make("level0", dict(blosc, clevel=0)), 0, 0, piece())
    assert not ok(make("b4096", dict(blosc, blocksize=4096)), 0, 0, piece())
    assert not ok(make("c60", chunk_shape=(8, 64, 60)), 0, 0, piece())
    assert not ok(make("u32", dtype=np.uint32), 0, 0, piece(dtype=torch.int32))
    assert not ok(make("fill5", fill=5), 0, 0, piece())
    assert not ok(default, 4, 0, piece(z=4))                 # starts off a chunk boundary in z
    assert not ok(default, 0, 32, piece(y=68))               # ... in y
    assert not ok(default, 0, 0, piece(z=4))                 # ends mid-chunk short of the array's end in z
    assert not ok(default, 0, 0, piece(y=96))                # ... in y
    assert not ok(default, 0, 0, piece(x=64))                # narrower than the array in x
    assert not ok(default, 0, 0, piece(x=256)[:, :, ::2])    # x stride 2
    monkeypatch.setenv("BSMI_DEVICE_FRAMES", "0")
    assert not ok(default, 0, 0, piece())
    monkeypatch.setenv("BSMI_DEVICE_FRAMES", "1")
    assert ok(default, 0, 0, piece())
