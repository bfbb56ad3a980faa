"""`bs refine morph` on the MI355X: the kernels of csrc/morph.hip bit-equal to the numpy restatement of the rule
(tests/morph_ref.py) -- there is no tolerance anywhere in this file -- and the driver end to end on a small store, seams
included."""
import ctypes as C

import numpy as np
import pytest

import morph_ref as R

pytestmark = pytest.mark.gpu

VOLUMES = {"block": ((13, 70, 101), 60, 11), "section": ((1, 33, 40), 14, 12)}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda(0)


def _host(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def volumes():
    out = {}
    for name, (shape, n, seed) in VOLUMES.items():
        a = R.cells(shape, n, seed)
        # the cases the rule is about really occur: ids above 2^32, ties between ids (in the 3-D and in the 2-D stencil), labels
        # that touch (so that they erode each other) and background next to them
        assert (a > np.uint64(1 << 32)).any() and (a == 0).any()
        assert R.tied_voxels(a) > 0 and sum(R.tied_voxels(s) for s in a) > 0
        assert ((a[:, :, 1:] != a[:, :, :-1]) & (a[:, :, 1:] != 0) & (a[:, :, :-1] != 0)).any()
        out[name] = a
    return out


@pytest.mark.parametrize("iterations", [1, 2, 5])
@pytest.mark.parametrize("xy", [False, True], ids=["3d", "xy"])
@pytest.mark.parametrize("op", ["dilate", "erode"])
@pytest.mark.parametrize("name", list(VOLUMES))
def test_stencil_ops_bit_equal_to_restatement(volumes, name, op, xy, iterations):
    from bootstrapper_amd import _lib
    from bootstrapper_amd.post.engine import label_morph
    a = volumes[name]
    src = _dev(a)
    got = _host(label_morph(src, _lib.MORPH_DILATE if op == "dilate" else _lib.MORPH_ERODE, iterations, xy))
    want = R.apply_block(a, op, iterations, xy)
    assert np.array_equal(_host(src), a)   # the input is never written
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:5])
    assert not np.array_equal(want, a)


def test_invalid_arguments_are_refused():
    import torch
    from bootstrapper_amd import _lib
    a, b, t = (torch.zeros((2, 4, 4), dtype=torch.int64, device="cuda:0") for _ in range(3))
    shape = _lib.i64x3(a.shape)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def call(src, op, n, dst, tmp):
        return _lib.lib.bsmi_label_morph_u64(0, src, shape, op, n, 0, dst, tmp, None)
    assert call(p(a), _lib.MORPH_ERODE, 1, p(b), None) == 0
    assert call(p(a), _lib.MORPH_DILATE, 2, p(b), p(t)) == 0
    assert call(p(a), 2, 1, p(b), None) == _lib.ERR_INVALID
    assert call(p(a), _lib.MORPH_ERODE, 0, p(b), p(t)) == _lib.ERR_INVALID
    assert call(p(a), _lib.MORPH_ERODE, 256, p(b), p(t)) == _lib.ERR_INVALID
    assert call(p(a), _lib.MORPH_ERODE, 1, p(a), None) == _lib.ERR_INVALID        # in place
    assert call(p(a), _lib.MORPH_ERODE, 2, p(b), None) == _lib.ERR_INVALID        # two iterations want the ping-pong buffer
    assert call(p(a), _lib.MORPH_ERODE, 2, p(b), p(a)) == _lib.ERR_INVALID
    assert call(None, _lib.MORPH_ERODE, 1, p(b), None) == _lib.ERR_INVALID
    assert call(p(a), _lib.MORPH_ERODE, 1, None, None) == _lib.ERR_INVALID
    assert b"null" in _lib.lib.bsmi_last_error()
    # fill_holes: in place, a table that is no power of two, too little scratch
    n = int(_lib.lib.bsmi_label_fill_holes_scratch_bytes(shape, 64))
    s = torch.empty(n, dtype=torch.uint8, device="cuda:0")

    def fill(src, dst, nbytes, cap):
        return _lib.lib.bsmi_label_fill_holes_u64(0, src, shape, 0, dst, p(s), nbytes, cap, None, None)
    assert fill(p(a), p(b), n, 64) == 0
    assert fill(p(a), p(a), n, 64) == _lib.ERR_INVALID
    assert fill(p(a), p(b), n, 48) == _lib.ERR_INVALID
    assert fill(p(a), p(b), n - 1, 64) == _lib.ERR_INVALID
    torch.cuda.synchronize()


def _fill(a, xy=False, **kw):
    from bootstrapper_amd.post.engine import label_fill_holes
    out, filled = label_fill_holes(_dev(a), xy, **kw)
    return _host(out), filled


def test_fill_holes_hand_made_cases():
    a = np.full((7, 9, 9), 4, np.uint64)
    a[3, 4, 4] = 0               # closed cavity
    a[3, 4, 0:3] = 0             # open to a face
    a[5, 6, 6] = 11              # enclosed foreign id
    got, filled = _fill(a)
    assert got[3, 4, 4] == 4 and (got[3, 4, 0:3] == 0).all() and got[5, 6, 6] == 4 and filled == 2
    assert np.array_equal(got, R.fill_holes(a))
    # 94 % and 96 % of the faces against one id
    for foreign, stays in ((6, True), (5, False)):
        c = R.contact_case(foreign)
        got, _ = _fill(c)
        assert np.array_equal(got, R.fill_holes(c))
        assert (got[2, 2, 3:28] == (0 if stays else 5)).all()
    # 3-D against per section: a column of background through every section
    b = np.full((3, 7, 7), 4, np.uint64)
    b[:, 3, 3] = 0
    assert np.array_equal(_fill(b)[0], b)
    assert (_fill(b, xy=True)[0] == 4).all()
    # no chaining: the inner hole takes the id its own neighbours had in the input
    c = np.full((1, 23, 23), 4, np.uint64)
    c[0, 2:21, 2:21] = 8
    c[0, 11, 11] = 0
    got, filled = _fill(c, xy=True)
    assert filled == 2 and got[0, 11, 11] == 8 and (got != 4).sum() == 1
    # the id 2^64 - 1 as a neighbour (the tables' empty marker has a slot of its own)
    d = np.full((5, 5, 5), np.uint64((1 << 64) - 1), np.uint64)
    d[2, 2, 2] = 0
    assert (_fill(d)[0] == np.uint64((1 << 64) - 1)).all()


@pytest.mark.parametrize("xy", [False, True], ids=["3d", "xy"])
@pytest.mark.parametrize("shape,seed", [((13, 70, 101), 21), ((1, 33, 40), 22), ((9, 64, 130), 23)])
def test_fill_holes_bit_equal_to_restatement(shape, seed, xy):
    a = R.holes(shape, seed)
    want = R.apply_block(a, "fill_holes", xy=xy)
    got, filled = _fill(a, xy)
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:5])
    if shape[0] == 1 and not xy:   # one section as a 3-D array: every voxel lies on a z face
        assert filled == 0 and np.array_equal(want, a)
    else:                          # some holes are filled, some components stay (cut by a face, or below 95 %)
        assert filled > 0 and not np.array_equal(want, a) and (want == 0).any()


def test_fill_holes_table_overflow_is_reported_and_the_wrapper_grows_the_table():
    import torch
    from bootstrapper_amd import _lib
    a = R.holes((13, 70, 101), 21)
    src, dst = _dev(a), _dev(np.zeros_like(a))
    shape = _lib.i64x3(a.shape)
    n = int(_lib.lib.bsmi_label_fill_holes_scratch_bytes(shape, 8))
    s = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    rc = _lib.lib.bsmi_label_fill_holes_u64(0, C.c_void_p(src.data_ptr()), shape, 0, C.c_void_p(dst.data_ptr()), C.c_void_p(s.data_ptr()), n, 8,
                                            None, None)
    assert rc == _lib.ERR_OVERFLOW and b"overflow" in _lib.lib.bsmi_last_error()
    got, _ = _fill(a, table_capacity=8)
    assert np.array_equal(got, R.fill_holes(a))


# ---- end to end ----

SHAPE, CHUNKS, BLOCK = (20, 90, 110), (8, 16, 16), 32


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    from bootstrapper_amd.zarr_io import prepare_ds
    root = str(tmp_path_factory.mktemp("morph") / "vol.zarr")
    vol = R.cells(SHAPE, 40, 31)
    rng = np.random.default_rng(32)
    for _ in range(80):          # cavities and specks for fill_holes, some of them across block seams
        lo = [int(rng.integers(0, s)) for s in SHAPE]
        vol[tuple(slice(o, o + int(rng.integers(1, 4))) for o in lo)] = 0 if rng.random() < 0.6 else 77
    ds = prepare_ds(root + "/seg", SHAPE, offset=(40, 8, 12), voxel_size=(4, 2, 2), chunk_shape=CHUNKS, dtype=np.uint64,
                    axis_names=["z", "y", "x"], units=["nm"] * 3)
    ds[:] = vol
    small = (vol % np.uint64(1000)).astype(np.uint32)
    d32 = prepare_ds(root + "/seg32", SHAPE, offset=(40, 8, 12), voxel_size=(4, 2, 2), chunk_shape=CHUNKS, dtype=np.uint32,
                     axis_names=["z", "y", "x"], units=["nm"] * 3)
    d32[:] = small
    return root, vol, small


@pytest.mark.parametrize("op,iterations,xy,context", [
    ("dilate", 2, False, 8), ("erode", 2, False, 8), ("opening", 2, False, 8), ("closing", 2, False, 8), ("fill_holes", 1, False, 8),
    ("dilate", 3, True, 8), ("closing", 1, True, 8), ("fill_holes", 1, True, 8),
    ("opening", 3, False, 1),    # the reach (6) is greater than the context: the seams must match the per-block restatement
])
def test_morph_end_to_end(store, op, iterations, xy, context):
    from bootstrapper_amd.refine import morph
    from bootstrapper_amd.zarr_io import open_ds
    root, vol, _ = store
    target = morph(root + "/seg", None if context == 8 and not xy else f"{root}/out_{op}_{int(xy)}_{context}", op=op, iterations=iterations, xy=xy,
                   context=context, block_size=BLOCK)
    if context == 8 and not xy:
        assert target == f"{root}/seg_{op}"
    out = open_ds(target)
    src = open_ds(root + "/seg")
    assert out.dtype == np.uint64 and tuple(out.shape) == SHAPE and tuple(out.chunks) == CHUNKS
    assert list(out.offset) == list(src.offset) == [40, 8, 12] and list(out.voxel_size) == [4, 2, 2]
    assert out.meta.get("compressor") == src.meta.get("compressor")
    want = R.morph_volume(vol, CHUNKS, op, iterations, xy, context, BLOCK)
    got = out[:]
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:5])
    assert not np.array_equal(want, vol)
    if context == 1:             # ... and they do differ from the whole-volume result there
        assert not np.array_equal(want, R.apply_block(vol, op, iterations, xy))
    assert np.array_equal(src[:], vol)


def test_other_integer_dtypes_keep_their_dtype(store):
    from bootstrapper_amd.refine import morph
    from bootstrapper_amd.zarr_io import open_ds
    root, _, small = store
    target = morph(root + "/seg32", op="closing", iterations=1, context=4, block_size=BLOCK)
    out = open_ds(target)
    assert target.endswith("seg32_closing") and out.dtype == np.uint32 and tuple(out.chunks) == CHUNKS
    want = R.morph_volume(small.astype(np.uint64), CHUNKS, "closing", 1, False, 4, BLOCK)
    assert np.array_equal(out[:], want.astype(np.uint32))


def test_through_the_command_line(store):
    from click.testing import CliRunner
    from bootstrapper_amd.cli import cli
    from bootstrapper_amd.zarr_io import open_ds
    root, vol, _ = store
    res = CliRunner().invoke(cli, ["refine", "morph", "-i", root + "/seg", "-o", root + "/cli_erode", "--op", "erode", "-n", "2", "--xy",
                                   "-c", "4", "-b", str(BLOCK), "-w", "3"])
    assert res.exit_code == 0, res.output
    assert "Writing to" in res.output
    assert np.array_equal(open_ds(root + "/cli_erode")[:], R.morph_volume(vol, CHUNKS, "erode", 2, True, 4, BLOCK))


def test_a_block_that_does_not_fit_names_block_size(store, monkeypatch):
    import click
    import torch
    from bootstrapper_amd.refine import morph
    root, _, _ = store
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1 << 16, 1 << 36))
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda *a, **k: 0)   # nothing cached by the allocator either
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda *a, **k: 0)
    with pytest.raises(click.ClickException, match="--block_size"):
        morph(root + "/seg", root + "/never", op="dilate", block_size=BLOCK)
    import os
    assert not os.path.exists(root + "/never")   # refused before anything is written
