"""`bs utils` on the MI355X: the kernels of csrc/utils.hip bit-equal to the numpy / scipy restatement (tests/utils_ref.py) -- there
is no tolerance anywhere in this file -- and the four drivers end to end on small stores, seams included."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import utils_ref as R

pytestmark = pytest.mark.gpu

# shape -> density of the set voxels
CLOSING_SHAPES = {(3, 70, 101): 0.01,    # two words per row, partial last word
                  (2, 45, 130): 0.02,    # three words per row
                  (2, 97, 64): 0.004,    # exactly one word; two tiles of rows
                  (1, 21, 23): 0.03,     # smaller than a word, H = 2 r + 1
                  (1, 5, 200): 0.02}     # H < r
SHAPE = (5, 37, 67)
FACTORS = [(1, 2, 2), (2, 2, 2), (3, 3, 3), (2, 3, 5)]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).cuda(0)


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _closing_input(shape, density):
    rng = np.random.default_rng(sum(shape))
    a = ((rng.random(shape) < density) * rng.integers(1, 256, shape)).astype(np.uint8)
    a[:, 0, 0] = a[:, 0, -1] = a[:, -1, 0] = a[:, -1, -1] = 200          # corners
    a[:, 0, shape[2] // 2] = a[:, -1, shape[2] // 3] = a[:, shape[1] // 2, 0] = a[:, shape[1] // 2, -1] = 3   # edges
    a[0, 1:4, 9:12] = 1   # a ring of eight around a hole of one voxel: every radius fills it
    a[0, 2, 10] = 0
    if shape[0] > 1:
        a[-1] = 0         # one empty section
    return a


@pytest.fixture(scope="module")
def closing_cases():
    cache = {}

    def get(shape, r):
        if shape not in cache:
            cache[shape] = (_closing_input(shape, CLOSING_SHAPES[shape]), {})
        a, want = cache[shape]
        if r not in want:
            want[r] = R.closing_volume(a, r)
            want[r].setflags(write=False)
        return a, want[r]
    return get


@pytest.mark.parametrize("r", [1, 3, 10])
@pytest.mark.parametrize("shape", list(CLOSING_SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_closing_bit_equal_to_restatement(closing_cases, shape, r):
    from bootstrapper_amd.utils import mask_closing
    a, want = closing_cases(shape, r)
    assert (a > 1).any() and not np.array_equal(want, (a != 0).astype(np.uint8)) and 0 < want.mean() < 1
    if shape[0] > 1:
        assert not want[-1].any()
    src = _cuda(a)
    got = _host(mask_closing(src, r), np.uint8)
    print(f"closing {shape} r={r}: mean {want.mean():.3f}, {int((got != want).sum())} voxels differ")
    assert np.array_equal(_host(src, np.uint8), a)   # the input is never written
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:5])


def test_closing_refuses_bad_arguments():
    import torch
    from bootstrapper_amd import _lib
    a = torch.zeros((2, 9, 70), dtype=torch.uint8, device="cuda:0")
    b = torch.zeros_like(a)
    shape = _lib.i64x3(a.shape)
    n = int(_lib.lib.bsmi_mask_closing_work_bytes(shape, 10))
    assert n == 2 * (9 + 20) * 2 * 8
    assert int(_lib.lib.bsmi_mask_closing_work_bytes(shape, 0)) == 0 and int(_lib.lib.bsmi_mask_closing_work_bytes(shape, 17)) == 0
    w = torch.zeros(n // 8, dtype=torch.int64, device="cuda:0")
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def call(src, r, dst, work, nbytes):
        return _lib.lib.bsmi_mask_closing_disk_u8(0, src, shape, r, dst, work, nbytes, None)
    assert call(p(a), 10, p(b), p(w), n) == 0
    assert call(p(a), 16, p(b), p(w), n) == _lib.ERR_INVALID          # the work buffer of r = 10 is short for r = 16
    assert call(p(a), 0, p(b), p(w), n) == _lib.ERR_INVALID
    assert call(p(a), 17, p(b), p(w), n) == _lib.ERR_INVALID
    assert b"radius" in _lib.lib.bsmi_last_error()
    assert call(p(a), 10, p(a), p(w), n) == _lib.ERR_INVALID           # in place
    assert call(p(a), 10, p(b), p(a), n) == _lib.ERR_INVALID
    assert call(p(a), 10, p(b), p(w), n - 8) == _lib.ERR_INVALID       # short work buffer
    assert b"work buffer" in _lib.lib.bsmi_last_error()
    assert call(None, 10, p(b), p(w), n) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    assert not _host(b, np.uint8).any()


def _scale_case(dtype, factor):
    """(array, lead, out_shape): a non-zero lead wherever the factor allows one"""
    rng = np.random.default_rng(sum(factor) + np.dtype(dtype).itemsize)
    top = np.iinfo(dtype).max
    if np.dtype(dtype).itemsize == 8:
        a = rng.integers(1, 1 << 40, SHAPE).astype(np.uint64) * np.uint64(1 << 20) + np.uint64(3)   # ids above 2^32
    else:
        a = rng.integers(0, int(top) + 1, SHAPE).astype(dtype)
    a[:, 8:30, 15:60] = top    # whole windows of the largest value
    lead = tuple(min(k - 1, 1 + (k > 3)) for k in factor)
    out_shape = tuple(-(-(n + l) // k) for n, l, k in zip(SHAPE, lead, factor))
    return a, lead, out_shape


@pytest.mark.parametrize("factor", FACTORS, ids=lambda f: "".join(map(str, f)))
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_downscale_mean_bit_equal_to_restatement(dtype, factor):
    from bootstrapper_amd.utils import rescale
    a, lead, out_shape = _scale_case(dtype, factor)
    want = R.downscale_mean(a, factor, lead, out_shape)
    assert any(lead) and (want == np.iinfo(dtype).max).any() and any(n % k for n, k in zip(SHAPE, factor))
    src = _cuda(a)
    got = _host(rescale(src, factor, lead, out_shape, "mean"), dtype)
    assert np.array_equal(_host(src, dtype), a)
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:5]


@pytest.mark.parametrize("factor", FACTORS, ids=lambda f: "".join(map(str, f)))
@pytest.mark.parametrize("dtype", [np.uint8, np.uint64])
def test_rescale_sample_bit_equal_to_restatement(dtype, factor):
    from bootstrapper_amd.utils import rescale
    a, lead, out_shape = _scale_case(dtype, factor)
    if dtype == np.uint64:
        assert (a > np.uint64(1 << 32)).all()
    src = _cuda(a)
    down = _host(rescale(src, factor, lead, out_shape, "down"), dtype)
    want = R.sample_down(a, factor, lead, out_shape)
    assert down.shape == want.shape and np.array_equal(down, want), np.argwhere(down != want)[:5]
    up_shape = tuple(n * k for n, k in zip(SHAPE, factor))
    up = _host(rescale(src, factor, (0, 0, 0), up_shape, "up"), dtype)
    assert np.array_equal(up, R.repeat_up(a, factor))
    assert np.array_equal(_host(src, dtype), a)


def test_scale_kernels_refuse_bad_arguments():
    import torch
    from bootstrapper_amd import _lib
    a = torch.zeros((2, 4, 6), dtype=torch.uint8, device="cuda:0")
    b = torch.zeros((2, 4, 6), dtype=torch.uint8, device="cuda:0")
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    i3, k3 = _lib.i64x3, lambda v: (C.c_int32 * 3)(*v)  # noqa: E731

    def mean(item, k, lead, src=a, dst=b):
        return _lib.lib.bsmi_downscale_mean(0, p(src), item, i3(a.shape), k3(k), k3(lead), p(dst), i3((1, 2, 3)), None)

    def sample(item, k, lead, mode, out_shape):
        return _lib.lib.bsmi_rescale_sample(0, p(a), item, i3(a.shape), k3(k), k3(lead), mode, p(b), i3(out_shape), None)
    assert mean(1, (2, 2, 2), (0, 1, 0)) == 0
    assert mean(4, (2, 2, 2), (0, 0, 0)) == _lib.ERR_INVALID           # averaging: u8 and u16 only
    assert mean(1, (2, 2, 2), (2, 0, 0)) == _lib.ERR_INVALID           # lead < factor
    assert mean(1, (0, 2, 2), (0, 0, 0)) == _lib.ERR_INVALID
    assert mean(1, (64, 64, 32), (0, 0, 0)) == _lib.ERR_INVALID        # a window above 65536 voxels
    assert mean(1, (2, 2, 2), (0, 0, 0), a, a) == _lib.ERR_INVALID     # in place
    assert sample(1, (1, 1, 1), (0, 0, 0), _lib.RESCALE_UP, (2, 4, 6)) == 0
    assert sample(1, (1, 1, 1), (0, 0, 0), _lib.RESCALE_UP, (2, 4, 7)) == _lib.ERR_INVALID   # more than in_shape * factor
    assert sample(1, (2, 2, 2), (0, 1, 0), _lib.RESCALE_UP, (2, 4, 6)) == _lib.ERR_INVALID
    assert sample(3, (2, 2, 2), (0, 0, 0), _lib.RESCALE_DOWN, (1, 2, 3)) == _lib.ERR_INVALID
    assert sample(1, (2, 2, 2), (0, 0, 0), 2, (1, 2, 3)) == _lib.ERR_INVALID
    torch.cuda.synchronize()


def _box(*tiles):
    from bootstrapper_amd.utils import new_box, nonzero_bbox
    import torch
    box = new_box(torch.device("cuda", 0))
    for a, origin in tiles:
        nonzero_bbox(_cuda(a), origin, box)
    return box.cpu().numpy().tolist()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.uint64])
def test_nonzero_bbox(dtype):
    big = np.iinfo(np.int64).max
    shape = (4, 9, 200)
    a = np.zeros(shape, dtype)
    assert _box((a, (0, 0, 0))) == [big, big, big, -1, -1, -1]           # all zero: the sentinel stays
    a[2, 5, 130] = np.iinfo(dtype).max
    assert _box((a, (0, 0, 0))) == [2, 5, 130, 2, 5, 130]                # a single voxel
    last = np.zeros(shape, dtype)
    last[-1, -1, -1] = 1
    assert _box((last, (0, 0, 0))) == [3, 8, 199, 3, 8, 199]             # only the last index of each axis
    faces = np.zeros(shape, dtype)
    faces[-1, 2, 70] = faces[1, -1, 64] = faces[0, 3, -1] = faces[1, 4, 63] = 1
    assert _box((faces, (0, 0, 0))) == [0, 2, 63, 3, 8, 199]
    rng = np.random.default_rng(5)
    b = ((rng.random(shape) < 0.01) * 7).astype(dtype)
    b[:, :2] = 0
    b[:, :, 150:] = 0
    sl = R.bbox(b)
    assert _box((b, (0, 0, 0))) == [s.start for s in sl] + [s.stop - 1 for s in sl]
    # two tiles of one volume, merged through their origins
    assert _box((a[:2], (10, 20, 30)), (a[2:], (12, 20, 30))) == [12, 25, 160, 12, 25, 160]
    assert _box((faces[:, :4], (0, 0, 0)), (faces[:, 4:], (0, 4, 0))) == [0, 2, 63, 3, 8, 199]


def test_bbox_refuses_bad_arguments():
    import torch
    from bootstrapper_amd import _lib
    a = torch.zeros((2, 4, 6), dtype=torch.uint8, device="cuda:0")
    box = torch.zeros(6, dtype=torch.int64, device="cuda:0")
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    assert _lib.lib.bsmi_nonzero_bbox(0, p(a), 3, _lib.i64x3(a.shape), _lib.i64x3((0, 0, 0)), p(box), None) == _lib.ERR_INVALID
    assert _lib.lib.bsmi_nonzero_bbox(0, p(a), 1, _lib.i64x3(a.shape), _lib.i64x3((0, -1, 0)), p(box), None) == _lib.ERR_INVALID
    assert _lib.lib.bsmi_nonzero_bbox(0, p(a), 1, _lib.i64x3(a.shape), _lib.i64x3((0, 0, 0)), None, None) == _lib.ERR_INVALID


# ---- the drivers, end to end ----

VOL, CHUNKS, OFFSET, VOXEL = (5, 70, 101), (2, 32, 32), (40, 4, 12), (40, 4, 4)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(77)
    raw = ((rng.random(VOL) < 0.012) * rng.integers(1, 256, VOL)).astype(np.uint8)
    raw[:, 0, 0] = raw[:, -1, -1] = 255
    labels = np.zeros(VOL, np.uint64)
    labels[1:4, 0:41, 30:61] = rng.integers(1, 6, (3, 41, 31)).astype(np.uint64) * np.uint64(1 << 33) + np.uint64(5)
    labels[1, 0:41, 30] = labels[3, 40, 30:61] = labels[2, 0, 60] = np.uint64(1 << 33) + np.uint64(5)
    raw.setflags(write=False)
    labels.setflags(write=False)
    return raw, labels


def _store(tmp_path_factory, name, **arrays):
    from bootstrapper_amd.zarr_io import prepare_ds
    root = str(tmp_path_factory.mktemp(name) / "vol.zarr")
    for ds, a in arrays.items():
        prepare_ds(f"{root}/{ds}", a.shape, offset=OFFSET, voxel_size=VOXEL, chunk_shape=CHUNKS, dtype=a.dtype, axis_names=["z", "y", "x"],
                   units=["nm"] * 3)[:] = a
    return root


def _same_geometry(out, dtype, shape=VOL, offset=OFFSET, voxel=VOXEL):
    assert out.dtype == dtype and tuple(out.shape) == tuple(shape) and tuple(out.chunks) == tuple(min(c, s) for c, s in zip(CHUNKS, shape))
    assert tuple(out.offset) == tuple(offset) and tuple(out.voxel_size) == tuple(voxel)
    assert out.axis_names == ["z", "y", "x"] and out.units == ["nm"] * 3


def test_mask_raw_equals_the_reference_block_grid(tmp_path_factory, data):
    from bootstrapper_amd.utils import mask
    from bootstrapper_amd.zarr_io import open_ds
    raw, _ = data
    root = _store(tmp_path_factory, "mask", raw=raw)
    target = mask(root + "/raw", mode="raw", tile=(32, 64))   # 3 x 2 tiles per chunk of sections: seams in y and in x
    assert target == root + "/raw_mask"
    out = open_ds(target)
    _same_geometry(out, np.uint8)
    want = R.mask_blockwise(raw, CHUNKS)
    got = out[:]
    assert 0 < want.mean() < 1 and not np.array_equal(want, raw != 0)
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:5])
    assert np.array_equal(open_ds(root + "/raw")[:], raw)
    # ... and with the default tile (the whole section) through the command line
    from click.testing import CliRunner
    from bootstrapper_amd.cli import cli
    res = CliRunner().invoke(cli, ["utils", "mask", "-i", root + "/raw", "-o", root + "/whole", "-m", "raw"])
    assert res.exit_code == 0 and "Writing mask to" in res.output, res.output
    assert np.array_equal(open_ds(root + "/whole")[:], want)


def test_mask_that_does_not_fit_is_refused(tmp_path_factory, data, monkeypatch):
    import click
    import torch
    from bootstrapper_amd.utils import mask
    root = _store(tmp_path_factory, "nofit", raw=data[0])
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1 << 12, 1 << 36))
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda *a, **k: 0)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda *a, **k: 0)
    with pytest.raises(click.ClickException, match="smaller tiles"):
        mask(root + "/raw", root + "/never", mode="raw")
    assert not os.path.exists(root + "/never")


def test_mask_labels(tmp_path_factory, data):
    from bootstrapper_amd.utils import mask
    from bootstrapper_amd.zarr_io import open_ds
    _, labels = data
    root = _store(tmp_path_factory, "lmask", labels=labels, labels32=(labels % np.uint64(97)).astype(np.uint32))
    for name in ("labels", "labels32"):
        target = mask(f"{root}/{name}", mode="labels")
        assert target == f"{root}/{name}".replace("labels", "labels_mask")
        out = open_ds(target)
        _same_geometry(out, np.uint8)
        want = (open_ds(f"{root}/{name}")[:] > 0).astype(np.uint8)
        assert 0 < want.mean() < 1 and np.array_equal(out[:], want)


def test_scale_pyramid_down_on_an_image(tmp_path_factory, data):
    from bootstrapper_amd.utils import scale_pyramid
    from bootstrapper_amd.zarr_io import open_ds
    raw, _ = data
    dense = (raw.astype(np.uint16) * 3 + np.arange(VOL[2], dtype=np.uint16) % 251).astype(np.uint8)
    root = _store(tmp_path_factory, "pyr", raw=dense)
    assert scale_pyramid(root + "/raw", ["1,2,2", "2 2 2"], mode="down") == root + "/raw"
    s0 = open_ds(root + "/raw/s0")
    _same_geometry(s0, np.uint8)
    assert np.array_equal(s0[:], dense) and not os.path.exists(root + "/raw__tmp") and os.path.exists(root + "/raw/.zgroup")
    s1, s2 = open_ds(root + "/raw/s1"), open_ds(root + "/raw/s2")
    _same_geometry(s1, np.uint8, (5, 36, 51), (40, 0, 8), (40, 8, 8))
    _same_geometry(s2, np.uint8, (3, 18, 26), (0, 0, 0), (80, 16, 16))
    want1 = R.downscale_mean(dense, (1, 2, 2), (0, 1, 1), (5, 36, 51))
    want2 = R.downscale_mean(want1, (2, 2, 2), (1, 0, 1), (3, 18, 26))
    assert want2.any() and np.array_equal(s1[:], want1) and np.array_equal(s2[:], want2)


def test_scale_pyramid_on_labels_down_and_up(tmp_path_factory, data):
    from bootstrapper_amd.utils import scale_pyramid
    from bootstrapper_amd.zarr_io import open_ds
    _, labels = data
    root = _store(tmp_path_factory, "lpyr", labels=labels, ids=labels)
    scale_pyramid(root + "/labels", ["1,2,2", "2,2,2"], chunk_shape="2,16,16", mode="down")
    s1, s2 = open_ds(root + "/labels/s1"), open_ds(root + "/labels/s2")
    assert s1.dtype == np.uint64 and tuple(s1.shape) == (5, 36, 51) and tuple(s1.chunks) == (2, 16, 16) and tuple(s1.offset) == (40, 0, 8)
    want1 = R.sample_down(labels, (1, 2, 2), (0, 1, 1), (5, 36, 51))
    want2 = R.sample_down(want1, (2, 2, 2), (1, 0, 1), (3, 18, 26))
    assert (want2 > np.uint64(1 << 32)).any() and np.array_equal(s1[:], want1) and np.array_equal(s2[:], want2)
    assert tuple(s2.voxel_size) == (80, 16, 16) and np.array_equal(open_ds(root + "/labels/s0")[:], labels)
    # up: the array becomes s1, s0 is the finer one
    scale_pyramid(root + "/ids", ["1,2,2"], mode="up")
    assert np.array_equal(open_ds(root + "/ids/s1")[:], labels)
    s0 = open_ds(root + "/ids/s0")
    _same_geometry(s0, np.uint64, (5, 140, 202), OFFSET, (40, 2, 2))
    assert np.array_equal(s0[:], R.repeat_up(labels, (1, 2, 2)))
    # ... and one more level from s0 has no room below: s0 -> s1 is refused because s1 exists
    import click
    with pytest.raises(click.ClickException, match="already exists"):
        scale_pyramid(root + "/ids/s0", ["1,2,2"], mode="up")


def test_bbox_pads_and_clips(tmp_path_factory, data):
    import click
    from bootstrapper_amd.utils import bbox
    from bootstrapper_amd.zarr_io import open_ds
    _, labels = data
    root = _store(tmp_path_factory, "bbox", labels=labels, empty=np.zeros(VOL, np.uint64))
    target = bbox(root + "/labels", padding=2)
    assert target == root + "/labels_bbox"
    sl = R.bbox(labels, 2)
    assert sl == (slice(0, 5), slice(0, 43), slice(28, 63))   # z and y clipped at 0, z at the far end too
    out = open_ds(target)
    assert out.dtype == np.uint64 and tuple(out.shape) == (5, 43, 35) and tuple(out.voxel_size) == VOXEL
    assert tuple(out.offset) == (40, 4, 12 + 28 * 4)
    assert np.array_equal(out[:], labels[sl])
    with pytest.raises(click.ClickException, match="no bounding box"):
        bbox(root + "/empty")
    assert not os.path.exists(root + "/empty_bbox")


def test_merge(tmp_path_factory, data):
    from click.testing import CliRunner
    from bootstrapper_amd.cli import cli
    from bootstrapper_amd.zarr_io import open_ds
    _, labels = data
    small = (labels >> np.uint64(33)).astype(np.uint32)
    root = _store(tmp_path_factory, "merge", seg=labels, seg32=small)
    ids = [int(v) for v in np.unique(labels) if v]
    assert len(ids) == 5
    merges = {str(ids[3]): [ids[0], ids[1]], str((1 << 40) + 1): [ids[1], ids[2]]}
    luts = os.path.join(os.path.dirname(root), "luts.json")
    with open(luts, "w") as f:
        json.dump({"merges": merges}, f)
    res = CliRunner().invoke(cli, ["utils", "merge", "-i", root + "/seg", "-l", luts])
    assert res.exit_code == 0 and "Writing to" in res.output, res.output
    out = open_ds(root + "/seg__merged.zarr")
    _same_geometry(out, np.uint64)
    want = R.merge(labels, merges)
    assert not np.array_equal(want, labels) and (want == np.uint64((1 << 40) + 1)).any() and np.array_equal(out[:], want)
    with open(luts, "w") as f:
        json.dump({"merges": {"77": [1, 2], "3": [2, 4]}}, f)
    res = CliRunner().invoke(cli, ["utils", "merge", "-i", root + "/seg32", "-o", root + "/m32", "-l", luts])
    assert res.exit_code == 0, res.output
    out = open_ds(root + "/m32")
    _same_geometry(out, np.uint64)
    assert np.array_equal(out[:], R.merge(small, {"77": [1, 2], "3": [2, 4]}))
