"""The rule of csrc/blosc_dev_u8.hip (tests/blosc_u8_ref.py) without a GPU: the restated frames read back through the strict
reader, the host codec, liblz4 and c-blosc; every clause of the rule is asserted from the sequences the reader finds; the header
is held to its fixed form; the rule's sizes on affinity-like data stay within 8 % of liblz4 and 8 % under what runs alone give; and
the gate of `bs predict` that sends a block's chunks to the device encoder has its truth table."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import blosc_ref as R
import blosc_u8_ref as U


@functools.lru_cache(maxsize=None)
def _cases():
    return U.byte_cases()


@functools.lru_cache(maxsize=None)
def _frame(name):
    return U.encode_frame_ref(_cases()[name])


NAMES = [
    "zeros", "const255", "noise", "A", "B", "bitmap", "far_and_near", "tie", "period3", "period300", "period5000", "end14", "end13", "end12",
    *[f"{w}{k}" for k in (1, 4, 11, 12, 13, 17, 300) for w in ("only", "last")]]


def test_the_names_are_the_cases():
    assert sorted(NAMES) == sorted(_cases())


@pytest.mark.parametrize("name", NAMES)
def test_strict_reader_and_host_codec_read_the_restated_frames(name):
    from bootstrapper_amd import _lib, codecs
    data = _cases()[name].tobytes()
    frame = _frame(name)
    got, info = U.frame_u8_strict(frame)
    assert got == data
    assert info["typesize"] == 1 and info["flags"] & ~2 == 0x30 and info["blocksize"] == min(U.BLOCK, len(data))
    for shuffle in (0, 1, 2):     # the dataset's shuffle setting does not matter to a reader: the frame's flags say none
        codec = _lib.Codec(_lib.CODEC_BLOSC, 5, _lib.BLOSC_LZ4, shuffle, 1, 0)
        assert codecs.decode(codec, frame, len(data)).tobytes() == data


@pytest.mark.parametrize("name", NAMES)
def test_liblz4_reads_every_block(name):
    lz = R.find_lz4()
    if lz is None:
        pytest.skip("no liblz4 on this machine")
    data = _cases()[name].tobytes()
    for at in range(0, len(data), U.BLOCK):
        blk = data[at:at + U.BLOCK]
        assert R.liblz4_decode(lz, U.lz4_stream_ref(blk), len(blk)) == blk


@pytest.mark.parametrize("name", NAMES)
def test_c_blosc_reads_the_restated_frames(name):
    lib = R.find_c_blosc()
    if lib is None:
        pytest.skip("no c-blosc on this machine")
    data = _cases()[name].tobytes()
    assert R.c_blosc_decode(lib, _frame(name), len(data)) == data


def test_noise_is_stored_and_constants_shrink_to_a_few_sequences():
    _, info = U.frame_u8_strict(_frame("noise"))
    assert info["stored"] and len(_frame("noise")) == 16 + _cases()["noise"].size
    for name in ("zeros", "const255"):
        assert len(_frame(name)) < 16 + 160 * 3     # per block: start, length, token, a literal, offset, 32 757 in 255-steps, 5 literals
        for n, seqs in U.frame_blocks(_frame(name)):
            assert seqs == ([(1, n - 6, 1)] if n >= 13 else None)


@pytest.mark.parametrize("k", (1, 4, 11, 12, 13, 17, 300))
def test_short_blocks(k):
    """up to 12 bytes no match may start (verbatim); from 13 on a run is one match from 1 to n - 5 (seen in the short last block)"""
    only = _frame(f"only{k}")
    _, info = U.frame_u8_strict(only)
    if k < 300:      # (from 13 on the block does shrink, by less than the 8 bytes of its start and length: the FRAME is stored)
        assert info["stored"] and len(only) == 16 + k
    else:
        assert U.frame_blocks(only) == [(k, [(1, k - 6, 1)])]
    blocks = U.frame_blocks(_frame(f"last{k}"))
    assert len(blocks) == 2 and blocks[0][0] == U.BLOCK and blocks[1] == (k, [(1, k - 6, 1)] if k >= 13 else None)


def test_a_repeat_300_on_is_matched_and_one_100_on_inside_a_group_is_not():
    (n, seqs), = U.frame_blocks(_frame("far_and_near"))
    far = [s for s in seqs if s[0] == 1600]
    assert len(far) == 1 and far[0][2] == 300 and 40 <= far[0][1] <= U.MAX_TABLE_LEN
    assert not [s for s in seqs if s[2] == 100] and not [s for s in seqs if 1126 <= s[0] < 1170]


def test_a_period_of_5000_becomes_consecutive_matches_of_68():
    (n, seqs), = U.frame_blocks(_frame("period5000"))
    assert max(ln for _, ln, _ in seqs) == U.MAX_TABLE_LEN
    pairs = [(a, b) for a, b in zip(seqs, seqs[1:]) if a[1] == b[1] == 68 and a[2] == b[2] == 5000 and a[0] + 68 == b[0]]
    assert len(pairs) >= 20
    assert sum(ln for _, ln, off in seqs if off == 5000 and ln == 68) > 0.5 * (n - 5000)


def test_equal_lengths_take_offset_1():
    (n, seqs), = U.frame_blocks(_frame("tie"))
    at = {s[0]: s for s in seqs}
    assert at[1015] == (1015, 89, 1)                     # the first run: nothing in the table yet
    assert at[1124] == (1124, 68, 1124 - 1023)           # the table match, cut at 68 (no run candidate at a run's first byte)
    assert at[1192] == (1192, 32, 1)                     # 32 bytes either way: offset 1
    length, offset = U.candidates(_cases()["tie"].tobytes())
    run_only, _ = U.candidates(_cases()["tie"].tobytes(), table=False)
    assert run_only[1192] == 32 and length[1192] == 32 and offset[1192] == 1


def test_no_match_starts_beyond_n_minus_12_or_ends_beyond_n_minus_5():
    n = 4096
    last = {k: U.frame_blocks(_frame(f"end{k}"))[0][1] for k in (14, 13, 12)}
    assert last[14][-1] == (n - 13, 8, 1)       # ends at n - 5 exactly
    assert last[13][-1] == (n - 12, 7, 1)       # starts at n - 12 exactly
    assert not last[12] or last[12][-1][0] < n - 12   # would start at n - 11: no match
    for name in NAMES:
        f = _frame(name)
        if U.frame_u8_strict(f)[1]["stored"]:
            continue
        for bn, seqs in U.frame_blocks(f):
            assert all(s <= bn - 12 and s + ln <= bn - 5 and 1 <= off <= s for s, ln, off in seqs or [])


def test_header_violations_are_rejected():
    frame = bytearray(_frame("last300"))
    U.frame_u8_strict(bytes(frame))
    for at, value in ((3, 8), (3, 0), (2, 0x31), (2, 0x20), (2, 0x34), (2, 0x10)):
        bad = bytearray(frame)
        bad[at] = value
        with pytest.raises(R.FormatError):
            U.frame_u8_strict(bytes(bad))
    bad = bytearray(frame)
    bad[16:20], bad[20:24] = frame[20:24], frame[16:20]     # the two block starts out of order
    with pytest.raises(R.FormatError):
        U.frame_u8_strict(bytes(bad))
    bad = bytearray(frame)
    bad[8:12] = (65536).to_bytes(4, "little")               # another block size
    with pytest.raises(R.FormatError):
        U.frame_u8_strict(bytes(bad))


def test_size_gate_against_liblz4_and_against_runs_alone():
    lz = R.find_lz4()
    if lz is None:
        pytest.skip("no liblz4 on this machine")
    lz.LZ4_compress_default.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    lz.LZ4_compress_default.restype = C.c_int
    sizes = {}
    for name in ("A", "B"):
        data = _cases()[name].tobytes()
        blocks = [data[at:at + U.BLOCK] for at in range(0, len(data), U.BLOCK)]
        dst = C.create_string_buffer(2 * U.BLOCK)
        sizes[name] = (sum(len(U.lz4_stream_ref(b)) for b in blocks), sum(lz.LZ4_compress_default(b, dst, len(b), 2 * U.BLOCK) for b in blocks),
                       sum(len(U.lz4_stream_ref(b, table=False)) for b in blocks))
        rule, lib, runs = sizes[name]
        print(f"fixture {name}: rule {rule} bytes, liblz4 {lib}, runs alone {runs}: {rule / lib:.3f} x liblz4, {rule / runs:.3f} x runs alone")
    rule, lib, runs = sizes["B"]
    assert rule <= 1.08 * lib
    assert rule <= 0.92 * runs


# ------------------------------------------------------------------------------------------------ the gate of bs predict
def _ds(shape=(6, 23, 50, 61), chunks=(6, 10, 32, 32), dtype=np.uint8, fill=0, sep=".", codec=None):
    from bootstrapper_amd import _lib
    codec = _lib.Codec(_lib.CODEC_BLOSC, 5, _lib.BLOSC_LZ4, 1, 1, 0) if codec is None else codec
    return types.SimpleNamespace(shape=shape, chunks=chunks, dtype=np.dtype(dtype), fill_value=fill, sep=sep, codec=codec)


def test_predict_gate_truth_table():
    from bootstrapper_amd import _lib
    from bootstrapper_amd.predict import pred_device_frames_refusal as why
    blk, hi = (10, 32, 0), (10, 18, 32)
    assert why(_ds(), blk, hi) is None
    assert why(_ds(), (20, 32, 32), (3, 18, 29)) is None                         # ends at the dataset's end on all axes
    for shuffle in (0, 1, 2):
        assert why(_ds(codec=_lib.Codec(_lib.CODEC_BLOSC, 5, _lib.BLOSC_LZ4, shuffle, 1, 0)), blk, hi) is None
    assert why(_ds(codec=_lib.Codec(_lib.CODEC_BLOSC, 9, _lib.BLOSC_LZ4, 1, 1, 32768)), blk, hi) is None
    assert why(_ds(fill=None), blk, hi) is None
    assert "lz4" in why(_ds(codec=_lib.Codec(_lib.CODEC_ZSTD, 1, 0, 0, 1, 0)), blk, hi)
    assert "lz4" in why(_ds(codec=_lib.Codec(_lib.CODEC_BLOSC, 5, _lib.BLOSC_ZSTD, 1, 1, 0)), blk, hi)
    assert "lz4" in why(_ds(codec=_lib.Codec(_lib.CODEC_RAW, 0, 0, 0, 1, 0)), blk, hi)
    assert "clevel" in why(_ds(codec=_lib.Codec(_lib.CODEC_BLOSC, 0, _lib.BLOSC_LZ4, 1, 1, 0)), blk, hi)
    assert "block size" in why(_ds(codec=_lib.Codec(_lib.CODEC_BLOSC, 5, _lib.BLOSC_LZ4, 1, 1, 65536)), blk, hi)
    assert "one byte" in why(_ds(dtype=np.uint16), blk, hi)
    assert "fill value" in why(_ds(fill=255), blk, hi)
    assert "nested" in why(_ds(sep="/"), blk, hi)
    assert "channels" in why(_ds(chunks=(3, 10, 32, 32)), blk, hi)
    assert "channels" in why(_ds(shape=(23, 50, 61), chunks=(10, 32, 32)), blk[:2], hi[:2])
    assert "1024 blocks" in why(_ds(shape=(6, 512, 512, 512), chunks=(6, 256, 256, 256)), (0, 0, 0), (256, 256, 256))
    assert why(_ds(shape=(1, 512, 512, 512), chunks=(1, 128, 512, 512)), (0, 0, 0), (128, 512, 512)) is None      # exactly 1024 blocks
    for off_grid in ((5, 32, 0), (10, 16, 0), (10, 32, 8)):
        assert "starts off" in why(_ds(), off_grid, (2, 2, 2))
    for short in ((9, 18, 32), (10, 17, 32), (10, 18, 31)):
        assert "ends off" in why(_ds(), blk, short)
    assert "ends off" in why(_ds(), blk, (0, 18, 32))
    assert why(_ds(chunks=(6, 1, 32, 32)), (16, 32, 0), (7, 18, 32)) is None     # a 2-D setup's stack of sections: 7 chunks deep


def test_predict_switches():
    from bootstrapper_amd import predict as P
    on = P.pred_device_frames_enabled
    assert on({}) is P.PRED_DEVICE_FRAMES_DEFAULT
    assert on({"BSMI_PRED_DEVICE_FRAMES": "1"}) is True and on({"BSMI_PRED_DEVICE_FRAMES": "0"}) is False
    assert on({"BSMI_DEVICE_FRAMES": "0", "BSMI_PRED_DEVICE_FRAMES": "1"}) is False       # the common switch turns both off
    assert on({"BSMI_DEVICE_FRAMES": "1"}) is P.PRED_DEVICE_FRAMES_DEFAULT
