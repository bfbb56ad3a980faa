"""The rule of csrc/blosc_dev_u8.hip (Blosc-1 frames of 1-byte items made on the device: the affinity chunks of `bs predict`),
restated sequentially.  The device frames are held byte-equal to `encode_frame_ref` by tests/test_blosc_u8_gpu.py; the readers are
those of tests/blosc_ref.py.

A frame: header {2, 1, flags, 1, nbytes, blocksize, cbytes}, flags 0x30 (lz4 format, blocks not split), blocksize
min(32 768, nbytes), the last block may be short; a frame that would not be smaller than nbytes + 16 is stored (flags 0x32).  A
block: 4-byte length + one LZ4 block, or the block's bytes when the LZ4 block would not be shorter.

The LZ4 block of b[0..n): every position i has at most two candidates,
  run    offset 1, length r(i) = the number of consecutive j >= i with b[j] == b[j-1] (i >= 1), a candidate from 5 bytes on;
  table  positions go in groups of 256; every position of a group looks up table[h(i)], h(i) = (le32(b, i) * 2654435761 mod 2^32)
         >> 20 (i + 4 <= n), as the table stood after all EARLIER groups, then the whole group enters itself with table[h] =
         max(table[h], i).  The match at offset i - c has the length of the common prefix of b[c..] and b[i..] cut at 68, a
         candidate from 4 bytes on.
No match starts beyond n - 12; every length is cut so that the match ends at or before n - 5 (a match cut below its minimum is no
candidate).  The longer candidate wins, offset 1 on equal length.  The parse is greedy from 0.

Not a test module."""
import numpy as np

from blosc_ref import _length_bytes  # noqa: F401  (the readers are imported by the tests from blosc_ref itself)

BLOCK = 32 * 1024
GROUP = 256
HASH_BITS = 12
MAX_TABLE_LEN = 68
MIN_RUN, MIN_TABLE = 5, 4
FLAGS = 0x30


def hashes(b):
    """h(i) of every i with i + 4 <= n"""
    a = np.frombuffer(bytes(b), np.uint8).astype(np.uint64)
    if a.size < 4:
        return np.zeros(0, np.int64)
    v = a[:-3] | a[1:-2] << np.uint64(8) | a[2:-1] << np.uint64(16) | a[3:] << np.uint64(24)
    return (((v * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(32 - HASH_BITS)).astype(np.int64)


def candidates(b, table=True):
    """(length, offset) of the winner at every position of the block, length 0 where there is none"""
    b = bytes(b)
    n = len(b)
    a = np.frombuffer(b, np.uint8)
    # r(i): distance to the next j >= i with b[j] != b[j-1] (or n)
    run = np.zeros(n, np.int64)
    nxt = n
    for i in range(n - 1, 0, -1):
        if a[i] != a[i - 1]:
            nxt = i
        run[i] = nxt - i
    h = hashes(b)
    tab = {}
    length, offset = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for g in range(0, n, GROUP):
        for i in range(g, min(n, g + GROUP)):
            if i > n - 12:
                break
            cap = n - 5 - i
            lr = min(int(run[i]), cap) if i >= 1 else 0
            if lr < MIN_RUN:
                lr = 0
            lt, c = 0, tab.get(int(h[i])) if table and i + 4 <= n else None
            if c is not None:
                lim = min(MAX_TABLE_LEN, cap)
                while lt < lim and b[c + lt] == b[i + lt]:
                    lt += 1
                if lt < MIN_TABLE:
                    lt = 0
            if lt > lr:
                length[i], offset[i] = lt, i - c
            elif lr:
                length[i], offset[i] = lr, 1
        for i in range(g, min(n - 3, g + GROUP)):   # after the whole group has looked
            tab[int(h[i])] = max(tab.get(int(h[i]), -1), i)
    return length, offset


def lz4_stream_ref(b, table=True):
    """the LZ4 block of b, whether or not it is shorter than b"""
    b = bytes(b)
    n = len(b)
    length, offset = candidates(b, table)
    out = bytearray()
    i = q = 0
    while i < n:
        ln = int(length[i])
        if not ln:
            i += 1
            continue
        lit, m4, off = i - q, ln - 4, int(offset[i])
        out.append(min(lit, 15) << 4 | min(m4, 15))
        if lit >= 15:
            out += _length_bytes(lit - 15)
        out += b[q:i]
        out += bytes([off & 255, off >> 8])
        if m4 >= 15:
            out += _length_bytes(m4 - 15)
        i = q = i + ln
    lit = n - q
    out.append(min(lit, 15) << 4)
    if lit >= 15:
        out += _length_bytes(lit - 15)
    out += b[q:]
    return bytes(out)


def encode_block_ref(b, table=True):
    """what the frame holds for one block behind its length: the LZ4 block, or the block itself when that is not shorter"""
    b = bytes(b)
    s = lz4_stream_ref(b, table)
    return s if len(s) < len(b) else b


def encode_frame_ref(chunk_u8, table=True):
    """the Blosc-1 frame of a uint8 chunk (C order, any size >= 1), as the device makes it"""
    data = np.ascontiguousarray(chunk_u8, dtype=np.uint8).tobytes()
    nbytes = len(data)
    assert nbytes >= 1
    bs = min(BLOCK, nbytes)
    blocks = []
    for at in range(0, nbytes, bs):
        enc = encode_block_ref(data[at:at + bs], table)
        blocks.append(len(enc).to_bytes(4, "little") + enc)
    nb = len(blocks)
    cbytes = 16 + 4 * nb + sum(len(x) for x in blocks)
    stored = cbytes >= nbytes + 16
    head = bytes([2, 1, FLAGS | (2 if stored else 0), 1]) + nbytes.to_bytes(4, "little") + bs.to_bytes(4, "little")
    if stored:
        return head + (nbytes + 16).to_bytes(4, "little") + data
    starts, at = bytearray(), 16 + 4 * nb
    for x in blocks:
        starts += at.to_bytes(4, "little")
        at += len(x)
    return head + cbytes.to_bytes(4, "little") + bytes(starts) + b"".join(blocks)


def frame_u8_strict(frame):
    """`blosc1_read_strict` for a frame made by this rule, whose header is fixed: typesize 1, flags exactly lz4 + not split
    (+ 2 only when stored), blocksize min(32 768, nbytes)"""
    from blosc_ref import FormatError, _le32, blosc1_read_strict
    frame = bytes(frame)
    if len(frame) < 16:
        raise FormatError("blosc: shorter than its header")
    if frame[3] != 1:
        raise FormatError(f"blosc: typesize {frame[3]}, not 1")
    if frame[2] & ~2 != FLAGS:
        raise FormatError(f"blosc: flags {frame[2]:#x}, not lz4 + blocks not split")
    nbytes, blocksize = _le32(frame, 4), _le32(frame, 8)
    if nbytes == 0 or blocksize != min(BLOCK, nbytes):
        raise FormatError(f"blosc: block size {blocksize} for {nbytes} bytes")
    data, info = blosc1_read_strict(frame)
    if len(data) != nbytes:
        raise FormatError("blosc: nbytes and the decoded size differ")
    return data, info


def parse_sequences(stream):
    """[(start, length, offset)] of the matches of an LZ4 block, in order (no checks: the strict reader makes those)"""
    stream = bytes(stream)
    out, ip, pos = [], 0, 0
    while ip < len(stream):
        token = stream[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            while True:
                lit += stream[ip]
                ip += 1
                if stream[ip - 1] != 255:
                    break
        ip += lit
        pos += lit
        if ip >= len(stream):
            break
        off = stream[ip] | stream[ip + 1] << 8
        ip += 2
        ml = token & 15
        if ml == 15:
            while True:
                ml += stream[ip]
                ip += 1
                if stream[ip - 1] != 255:
                    break
        out.append((pos, ml + 4, off))
        pos += ml + 4
    return out


def frame_blocks(frame):
    """the blocks of a frame that is not stored -> [(block bytes n, matches [(start, length, offset)] or None where verbatim)]"""
    frame = bytes(frame)
    _, info = frame_u8_strict(frame)
    assert not info["stored"]
    out = []
    for b, (at, lens, traces) in enumerate(zip(info["starts"], info["lengths"], info["traces"])):
        n = min(info["blocksize"], info["nbytes"] - b * info["blocksize"])
        out.append((n, None if traces[0] is None else parse_sequences(frame[at + 4:at + 4 + lens[0]])))
    return out


def _distinct(rng, n):
    """n random bytes of which none equals the one before it: a background without a single run"""
    return ((int(rng.integers(0, 256)) + np.cumsum(rng.integers(1, 256, size=n, dtype=np.int64))) % 256).astype(np.uint8)


def far_and_near():
    """a background without runs, 40 bytes of it repeated 300 bytes on (across a group border: found) and another 40 bytes
    repeated 100 bytes on INSIDE one group of 256 (not found)"""
    a = _distinct(np.random.default_rng(11), 4096)
    a[1600:1640] = a[1300:1340]     # groups [1280, 1536) -> [1536, 1792)
    a[1130:1170] = a[1030:1070]     # both in group [1024, 1280)
    return a


def tie_case():
    """a run of 0x77 across the group border at 1024 (so that the table knows position 1023 with 80 more of them behind it), then
    in the same group a run of 100: its first position takes the table match cut at 68, and at the 69th both candidates have 32"""
    a = _distinct(np.random.default_rng(12), 4096)
    a[a == 0x77] = 0x78
    a[1:][a[1:] == a[:-1]] ^= 0x10                   # (the replacement may have made a pair)
    a[1014:1104] = 0x77
    a[1124:1224] = 0x77
    return a


def end_cases(n=4096):
    """{k: block whose last k bytes are one value behind 2000 zeros and a background without runs}: the run candidate of the position behind
    the run's first byte starts at n - k + 1"""
    out = {}
    for k in (14, 13, 12):
        a = _distinct(np.random.default_rng(13), n)
        a[a == 0x55] = 0x56
        a[1:][a[1:] == a[:-1]] ^= 0x10
        a[n - k:] = 0x55
        a[:2000] = 0                # (so that the frame is not a stored one)
        out[k] = a
    return out


def byte_cases():
    """{name: uint8 array}: the inputs that the CPU and the GPU tests share"""
    rng = np.random.default_rng(7)
    out = {"zeros": np.zeros(2 * BLOCK + 1000, np.uint8), "const255": np.full(BLOCK + 13, 255, np.uint8),
           "noise": rng.integers(0, 256, size=2 * BLOCK + 17, dtype=np.uint8),
           "A": fixture_a().reshape(-1), "B": fixture_b().reshape(-1),
           "bitmap": np.where(rng.random(BLOCK + 5000) < 0.5, 0, 255).astype(np.uint8),
           "far_and_near": far_and_near(), "tie": tie_case()}
    for p in (3, 300, 5000):
        out[f"period{p}"] = np.tile(rng.integers(0, 256, size=p, dtype=np.uint8), 2 * BLOCK // p + 1)[:BLOCK + 777 if p != 5000 else BLOCK]
    for k, a in end_cases().items():
        out[f"end{k}"] = a
    for k in (1, 4, 11, 12, 13, 17, 300):
        out[f"only{k}"] = np.full(k, 9, np.uint8)                                         # a chunk's only block
        out[f"last{k}"] = np.concatenate([fixture_a().reshape(-1)[:BLOCK], np.full(k, 9, np.uint8)])   # ... and its short last one
    return out


def fixture(gain, noise, seed):
    """F(gain, noise, seed): 131 072 bytes of affinity-like data (saturating inside objects, dropping at boundaries), four blocks"""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    shape = (8, 128, 128)
    g = gaussian_filter(rng.standard_normal(shape), (1, 4, 4))
    g = g / g.std()
    x = gain * (np.abs(g) - 0.3) + noise * rng.standard_normal(shape)
    return np.floor(255.0 / (1.0 + np.exp(-x))).astype(np.uint8)


def fixture_a():
    return fixture(12, 1.0, 1)


def fixture_b():
    return fixture(40, 2.0, 2)
