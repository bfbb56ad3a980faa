"""The Blosc-1 / LZ4 block formats in plain Python, for the frames that csrc/blosc_dev.hip makes on the device (and, as a reader,
for every lz4 frame of csrc/chunk_codec.cpp and of c-blosc):

  * `lz4_block_strict` / `blosc1_read_strict` / `blosc1_frame_strict`: readers that ENFORCE the formats -- the end-of-block rules of
    the LZ4 block format (lz4 Block Format Description 1.6: "the last sequence contains only literals", "the last 5 bytes of input
    are always literals", "the last match must start at least 12 bytes before the end of block"), offsets inside the output, input
    and output consumed exactly; Blosc's header, its block-start table and a tiling of the frame by the length-prefixed splits with
    no gap and no overlap.  The host codec's `lz4_decode` checks none of the end-of-block rules and neither the version bytes nor
    the order of the block starts.
  * `encode_plane_ref` / `encode_frame_ref`: the sequential restatement of the rule in blosc_dev.hip's header comment.  The device
    frames are held byte-equal to it by tests/test_blosc_dev_edges_gpu.py.

Not a test module."""
import ctypes as C
import ctypes.util
import os
import sys

import numpy as np

BLOCK = 256 * 1024          # Blosc block size of the device frames
PLANE = BLOCK // 8          # bytes of one byte plane of a block
MIN_RUN = 8                 # shortest run that becomes a match
REAL_BLOSC = "/opt/conda/lib/libblosc.so.1"


class FormatError(ValueError):
    """a stream or a frame breaks its format"""


# ------------------------------------------------------------------------------------------------ readers
def lz4_block_strict(src, n):
    """decode the LZ4 block `src` that must hold exactly `n` bytes -> (bytes, trace); trace = [(literal count, match length)] per
    sequence, match length 0 for the closing literals.  Raises FormatError for anything the block format forbids."""
    src = bytes(src)
    out = bytearray()
    trace = []
    ip, end = 0, len(src)
    if end == 0:
        raise FormatError("lz4: empty stream (even an empty block has its token)")
    while True:
        if ip >= end:
            raise FormatError("lz4: the stream ends after a match: the last sequence must be literals only")
        token = src[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            while True:
                if ip >= end:
                    raise FormatError("lz4: literal length runs past the input")
                s = src[ip]
                ip += 1
                lit += s
                if s != 255:
                    break
        if lit > end - ip:
            raise FormatError("lz4: literals run past the input")
        if len(out) + lit > n:
            raise FormatError(f"lz4: literals run past the {n} bytes of the block")
        out += src[ip:ip + lit]
        ip += lit
        if ip == end:                      # the closing literals
            if token & 15:
                raise FormatError("lz4: the last token names a match length but no match follows")
            trace.append((lit, 0))
            break
        if end - ip < 2:
            raise FormatError("lz4: offset runs past the input")
        off = src[ip] | (src[ip + 1] << 8)
        ip += 2
        ml = token & 15
        if ml == 15:
            while True:
                if ip >= end:
                    raise FormatError("lz4: match length runs past the input")
                s = src[ip]
                ip += 1
                ml += s
                if s != 255:
                    break
        ml += 4
        pos = len(out)
        if off == 0:
            raise FormatError("lz4: offset 0")
        if off > pos:
            raise FormatError(f"lz4: offset {off} reaches before the block's start ({pos} bytes produced)")
        if pos > n - 12:
            raise FormatError(f"lz4: a match starts at {pos}, inside the last 12 bytes of {n}")
        if pos + ml > n - 5:
            raise FormatError(f"lz4: a match ends at {pos + ml}, inside the last 5 bytes of {n}")
        if off >= ml:
            out += out[pos - off:pos - off + ml]
        elif off == 1:
            out += bytes(out[pos - 1:pos]) * ml
        else:
            pat = bytes(out[pos - off:pos])
            out += (pat * (ml // off + 1))[:ml]
        trace.append((lit, ml))
    if len(out) != n:
        raise FormatError(f"lz4: {len(out)} bytes came out, {n} were expected")
    return bytes(out), trace


def _le32(b, at):
    return int.from_bytes(b[at:at + 4], "little")


def _unshuffle(block, ts):
    """undo c-blosc's byte shuffle of one block: whole elements transposed, the bytes beyond them in place"""
    a = np.frombuffer(block, np.uint8)
    ne = a.size // ts
    body = a[:ne * ts].reshape(ts, ne).T.reshape(-1)
    return body.tobytes() + a[ne * ts:].tobytes()


def blosc1_read_strict(frame):
    """decode a Blosc-1 frame whose inner codec is lz4 (or lz4hc: the same format) and whose shuffle is none or byte, typesize and
    blocksize from its header -> (bytes, info).  Enforced: version bytes 2 and 1, cbytes == len(frame), a stored frame of exactly
    16 + nbytes bytes, an ascending block-start table that begins right behind itself, the length-prefixed splits of every block
    tiling the frame up to cbytes, every split through `lz4_block_strict` unless its length is the split's size (verbatim).
    info: flags, typesize, nbytes, blocksize, cbytes, stored, starts, lengths [block][split], traces [block][split] (None: verbatim)."""
    frame = bytes(frame)
    if len(frame) < 16:
        raise FormatError("blosc: shorter than its header")
    if frame[0] != 2 or frame[1] != 1:
        raise FormatError(f"blosc: version bytes {frame[0]}, {frame[1]} (2, 1 expected)")
    flags, ts = frame[2], frame[3] or 1
    nbytes, blocksize, cbytes = _le32(frame, 4), _le32(frame, 8), _le32(frame, 12)
    if cbytes != len(frame):
        raise FormatError(f"blosc: cbytes {cbytes} but the frame has {len(frame)} bytes")
    if flags & 4:
        raise FormatError("blosc: bit shuffle is not restated here")
    if flags & 0x88:
        raise FormatError(f"blosc: reserved flag bits set ({flags:#x})")
    if flags >> 5 != 1:
        raise FormatError(f"blosc: inner codec format {flags >> 5}, not lz4")
    info = {"flags": flags, "typesize": ts, "nbytes": nbytes, "blocksize": blocksize, "cbytes": cbytes, "stored": bool(flags & 2),
            "starts": [], "lengths": [], "traces": []}
    if flags & 2:
        if len(frame) != 16 + nbytes:
            raise FormatError(f"blosc: a stored frame of {nbytes} bytes has {len(frame)} bytes, not {16 + nbytes}")
        return frame[16:], info
    if nbytes == 0:
        if len(frame) != 16:
            raise FormatError("blosc: an empty frame with bytes behind its header")
        return b"", info
    if blocksize == 0 or blocksize > nbytes:
        raise FormatError(f"blosc: block size {blocksize} for {nbytes} bytes")
    nblocks = -(-nbytes // blocksize)
    at = 16 + 4 * nblocks
    if at > len(frame):
        raise FormatError("blosc: the block-start table is cut off")
    starts = [_le32(frame, 16 + 4 * b) for b in range(nblocks)]
    info["starts"] = starts
    if starts[0] != at:
        raise FormatError(f"blosc: the first block starts at {starts[0]}, not right behind the table ({at})")
    if any(b <= a for a, b in zip(starts, starts[1:])):
        raise FormatError("blosc: block starts do not ascend")
    out = []
    for b in range(nblocks):
        if starts[b] != at:
            raise FormatError(f"blosc: block {b} starts at {starts[b]}, the block before it ends at {at}")
        short = b == nblocks - 1 and nbytes % blocksize
        bsize = nbytes % blocksize if short else blocksize
        nsplits = ts if (not flags & 16 and ts <= 16 and blocksize // ts >= 128 and not short) else 1
        ne = bsize // nsplits
        parts, lens, traces = [], [], []
        for _ in range(nsplits):
            if at + 4 > cbytes:
                raise FormatError(f"blosc: block {b} runs past the frame")
            cb = _le32(frame, at)
            at += 4
            if cb > cbytes - at:
                raise FormatError(f"blosc: block {b} runs past the frame")
            if cb > ne:
                raise FormatError(f"blosc: a split of {ne} bytes takes {cb}")
            if cb == ne:
                parts.append(frame[at:at + cb])
                traces.append(None)
            else:
                data, tr = lz4_block_strict(frame[at:at + cb], ne)
                parts.append(data)
                traces.append(tr)
            lens.append(cb)
            at += cb
        info["lengths"].append(lens)
        info["traces"].append(traces)
        block = b"".join(parts)
        out.append(_unshuffle(block, ts) if flags & 1 and ts > 1 else block)
    if at != cbytes:
        raise FormatError(f"blosc: the blocks end at {at}, the frame at {cbytes}")
    return b"".join(out), info


def blosc1_frame_strict(frame, typesize=8):
    """`blosc1_read_strict` for a frame made on the device, whose header is fixed: flags exactly byte shuffle + lz4 (+ 2 only
    when stored: split blocks, so 16 is NOT set), the given typesize, blocks of 256 KiB, whole blocks only."""
    frame = bytes(frame)
    if len(frame) < 16:
        raise FormatError("blosc: shorter than its header")
    if frame[0] != 2 or frame[1] != 1:
        raise FormatError(f"blosc: version bytes {frame[0]}, {frame[1]} (2, 1 expected)")
    flags, nbytes, blocksize = frame[2], _le32(frame, 4), _le32(frame, 8)
    if flags & 4:
        raise FormatError("blosc: bit shuffle")
    if flags >> 5 != 1:
        raise FormatError(f"blosc: inner codec format {flags >> 5}, not lz4")
    if flags & ~2 != (1 | 1 << 5):
        raise FormatError(f"blosc: flags {flags:#x}, not byte shuffle + lz4")
    if frame[3] != typesize:
        raise FormatError(f"blosc: typesize {frame[3]}, not {typesize}")
    if blocksize != BLOCK:
        raise FormatError(f"blosc: block size {blocksize}, not {BLOCK}")
    if nbytes == 0 or nbytes % BLOCK:
        raise FormatError(f"blosc: {nbytes} bytes are not whole blocks")
    data, info = blosc1_read_strict(frame)
    if len(data) != nbytes:
        raise FormatError("blosc: nbytes and the decoded size differ")
    return data, info


# ------------------------------------------------------------------------------------------------ the encoder's rule, restated
def _length_bytes(v):
    """the bytes that continue a length field of 15: v = length - 15 in 255-steps"""
    return b"\xff" * (v // 255) + bytes([v % 255])


def plane_runs(plane):
    """(starts, lengths) of the runs of the plane: a run starts at 0, at every byte that differs from the one before it, and at
    every one of the last 12 bytes (so no match reaches into them)"""
    s = np.frombuffer(bytes(plane), np.uint8)
    n = s.size
    st = np.ones(n, bool)
    st[1:] = s[1:] != s[:-1]
    st[max(0, n - 12):] = True
    starts = np.flatnonzero(st)
    return starts, np.diff(np.append(starts, n))


def plane_stream_ref(plane):
    """the LZ4 block of the plane whether or not it is shorter than the plane: every run of at least 8 bytes is one sequence --
    literals from the end of the run before it up to and including its own first byte, a match of the rest at offset 1 -- and the
    closing literals follow"""
    plane = bytes(plane)
    starts, lengths = plane_runs(plane)
    out = bytearray()
    q = 0
    for p, ln in zip(starts[lengths >= MIN_RUN].tolist(), lengths[lengths >= MIN_RUN].tolist()):
        lit, m4 = p - q + 1, ln - 1 - 4
        out.append(min(lit, 15) << 4 | min(m4, 15))
        if lit >= 15:
            out += _length_bytes(lit - 15)
        out += plane[q:q + lit]
        out += b"\x01\x00"
        if m4 >= 15:
            out += _length_bytes(m4 - 15)
        q = p + ln
    lit = len(plane) - q
    out.append(min(lit, 15) << 4)
    if lit >= 15:
        out += _length_bytes(lit - 15)
    out += plane[q:]
    return bytes(out)


def encode_plane_ref(plane):
    """what the frame holds for one byte plane: its LZ4 block, or the plane itself when the block would not be shorter"""
    plane = bytes(plane)
    stream = plane_stream_ref(plane)
    return stream if len(stream) < len(plane) else plane


def encode_frame_ref(chunk_u64):
    """the Blosc-1 frame of a uint64 chunk of whole 256 KiB blocks (C order), as the device makes it"""
    flat = np.ascontiguousarray(chunk_u64, dtype=np.uint64).reshape(-1)
    nbytes = flat.size * 8
    assert nbytes and nbytes % BLOCK == 0
    nb = nbytes // BLOCK
    by = flat.view(np.uint8).reshape(nb, PLANE, 8)
    blocks = []
    for b in range(nb):
        body = bytearray()
        for p in range(8):
            enc = encode_plane_ref(by[b, :, p].tobytes())
            body += len(enc).to_bytes(4, "little") + enc
        blocks.append(bytes(body))
    cbytes = 16 + 4 * nb + sum(len(b) for b in blocks)
    stored = cbytes >= nbytes + 16
    head = bytes([2, 1, (2 if stored else 0) | 1 | 1 << 5, 8])
    if stored:
        return head + nbytes.to_bytes(4, "little") + BLOCK.to_bytes(4, "little") + (nbytes + 16).to_bytes(4, "little") + flat.tobytes()
    table, at = bytearray(), 16 + 4 * nb
    for b in blocks:
        table += at.to_bytes(4, "little")
        at += len(b)
    return head + nbytes.to_bytes(4, "little") + BLOCK.to_bytes(4, "little") + cbytes.to_bytes(4, "little") + bytes(table) + b"".join(blocks)


def planes_to_u64(patterns):
    """8 byte patterns of 32 768 bytes -> uint64[32768] whose element e carries pattern p's byte e in its byte p: as a one-block
    chunk (8, 64, 64) it has exactly those 8 planes"""
    assert len(patterns) == 8
    out = np.zeros(PLANE, np.uint64)
    for p, pat in enumerate(patterns):
        a = np.frombuffer(bytes(pat), np.uint8)
        assert a.size == PLANE
        out |= a.astype(np.uint64) << np.uint64(8 * p)
    return out


def distinct_bytes(rng, n, avoid=None):
    """n random bytes of which none equals the one before it (nor `avoid` at the front): a background without a single run"""
    step = rng.integers(1, 256, size=n, dtype=np.int64)
    first = int(rng.integers(0, 256)) if avoid is None else int(avoid)
    return ((first + np.cumsum(step)) % 256).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ third-party readers
def find_lz4():
    """liblz4 through ctypes, or None where the machine has none"""
    name = ctypes.util.find_library("lz4")
    for cand in ([name] if name else []) + [os.path.join(sys.prefix, "lib", "liblz4.so.1")]:
        try:
            lib = C.CDLL(cand)
        except OSError:
            continue
        lib.LZ4_decompress_safe.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
        lib.LZ4_decompress_safe.restype = C.c_int
        return lib
    return None


def find_c_blosc():
    """c-blosc through ctypes, or None where the machine has none"""
    name = ctypes.util.find_library("blosc")
    for cand in ([name] if name else []) + [os.path.join(sys.prefix, "lib", "libblosc.so.1"), REAL_BLOSC]:
        try:
            lib = C.CDLL(cand)
        except OSError:
            continue
        lib.blosc_decompress_ctx.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.c_int]
        lib.blosc_decompress_ctx.restype = C.c_int
        return lib
    return None


def liblz4_decode(lib, stream, n):
    """LZ4_decompress_safe of one block -> bytes (raises FormatError where liblz4 refuses it)"""
    dst = C.create_string_buffer(n + 1)
    r = lib.LZ4_decompress_safe(bytes(stream), dst, len(stream), n)
    if r != n:
        raise FormatError(f"liblz4: LZ4_decompress_safe gave {r} for a block of {n}")
    return dst.raw[:n]


def c_blosc_decode(lib, frame, n):
    """blosc_decompress_ctx of one frame with one thread -> bytes (raises FormatError where c-blosc refuses it)"""
    dst = C.create_string_buffer(n + 1)
    r = lib.blosc_decompress_ctx(bytes(frame), dst, n, 1)
    if r != n:
        raise FormatError(f"c-blosc: blosc_decompress_ctx gave {r} for a frame of {n}")
    return dst.raw[:n]
