"""`bs refine morph` without a GPU: the numpy restatement of the rule (tests/morph_ref.py) against scipy on single-id volumes and
against hand-made cases, the block grid against hand-written lists, the per-block driver against the whole-volume form, and
the command line."""
import numpy as np
import pytest
from click.testing import CliRunner
from scipy import ndimage

import morph_ref as R

from bootstrapper_amd import refine as RF


def _blobs(shape, seed, p=0.35):
    rng = np.random.default_rng(seed)
    a = ndimage.binary_opening(rng.random(shape) < p, iterations=1) | (rng.random(shape) < 0.03)
    return a


@pytest.mark.parametrize("shape", [(9, 24, 31), (1, 20, 27), (22, 29)])
@pytest.mark.parametrize("n", [1, 3])
def test_single_id_volumes_equal_scipy_binary_morphology(shape, n):
    fg = _blobs(shape, 7 + len(shape))
    full = np.ones((3,) * len(shape), bool)
    lab = fg.astype(np.uint64) * np.uint64((1 << 40) + 5)
    d = R.apply_array(lab, "dilate", n)
    e = R.apply_array(lab, "erode", n)
    assert np.array_equal(d != 0, ndimage.binary_dilation(fg, structure=full, iterations=n))
    assert np.array_equal(e != 0, ndimage.binary_erosion(fg, structure=full, iterations=n, border_value=0))
    assert set(np.unique(d)) <= {0, (1 << 40) + 5} and set(np.unique(e)) <= {0, (1 << 40) + 5}
    assert fg.any() and not fg.all() and (e != 0).sum() < fg.sum() < (d != 0).sum()


def test_dilate_most_frequent_id_and_ties_to_the_smallest():
    a = np.zeros((3, 5), np.uint64)
    a[0, 0:2] = 9
    a[2, 0] = 4
    a[0, 4] = 7
    a[2, 4] = 3
    d = R.dilate_step(a)
    assert d[1, 1] == 9          # 9 twice, 4 once
    assert d[1, 0] == 9
    assert d[1, 3] == 3 and d[1, 4] == 3   # 7 and 3 once each: the smallest
    assert d[1, 2] == 9          # sees 9 at (0, 1) only
    assert d[2, 2] == 0          # no labelled neighbour: stays 0
    assert R.tied_voxels(a) == 2
    # in 3-D the stencil is 3 x 3 x 3: a diagonal neighbour counts, one two voxels away does not
    b = np.zeros((3, 3, 4), np.uint64)
    b[0, 0, 0] = 5
    d3 = R.dilate_step(b)
    assert d3[1, 1, 1] == 5 and d3[1, 1, 2] == 0 and d3[2, 2, 2] == 0


def test_dilate_leaves_labelled_voxels_alone():
    a = np.full((5, 5), 2, np.uint64)
    a[2, 2] = 8                  # surrounded by eight 2s: background_only keeps it
    a[0, 0] = 0
    d = R.dilate_step(a)
    assert d[2, 2] == 8 and d[0, 0] == 2 and np.array_equal(d[a != 0], a[a != 0])


def test_labels_erode_each_other_and_faces_always_go():
    a = np.zeros((7, 12), np.uint64)
    a[:, :6] = 1
    a[:, 6:] = 2
    e = R.erode_step(a)
    want = np.zeros_like(a)
    want[1:6, 1:5] = 1           # the column next to label 2 goes, and so does everything on the array's edges
    want[1:6, 7:11] = 2
    assert np.array_equal(e, want)
    assert not R.apply_array(a, "erode", 3)[:, 4:8].any()
    # one section of a 3-D block: every voxel lies on a z face
    assert not R.erode_step(np.full((1, 6, 6), 3, np.uint64)).any()
    assert R.apply_block(np.full((1, 6, 6), 3, np.uint64), "erode", 1, xy=True)[0, 1:5, 1:5].all()


def test_fill_holes_threshold_on_both_sides():
    lo, hi = R.contact_case(6), R.contact_case(5)     # 96 / 102 = 94.1 %, 97 / 102 = 95.1 %
    assert 20 * 96 < 19 * 102 and 20 * 97 >= 19 * 102
    f_lo, f_hi = R.fill_holes(lo), R.fill_holes(hi)
    assert (f_lo[2, 2, 3:28] == 0).all()
    assert (f_hi[2, 2, 3:28] == 5).all()
    # the voxels of 6 are enclosed components of their own: five faces against 5, one against 0 -> 5 / 6 < 0.95, kept
    assert (f_hi == 6).sum() == 5 and (f_lo == 6).sum() == 6
    exact = np.full((3, 5, 22), 5, np.uint64)       # T = 20 in 2-D sections: 19 / 20 is the boundary itself
    exact[1, 2, 1:10] = 0                           # 9 voxels in a row: 2 * 9 + 2 = 20 faces
    exact[1, 1, 4] = 6
    assert (R.apply_block(exact, "fill_holes", xy=True)[1, 2, 1:10] == 5).all()
    exact[1, 3, 6] = 6                              # 18 / 20
    assert (R.apply_block(exact, "fill_holes", xy=True)[1, 2, 1:10] == 0).all()


def test_fill_holes_faces_foreign_ids_and_no_chaining():
    a = np.full((7, 9, 9), 4, np.uint64)
    a[3, 4, 4] = 0               # closed cavity
    a[3, 4, 0:3] = 0             # open to a face
    a[5, 6, 6] = 11              # enclosed foreign id
    f = R.fill_holes(a)
    assert f[3, 4, 4] == 4 and (f[3, 4, 0:3] == 0).all() and f[5, 6, 6] == 4
    # 3-D: a section's hole that is open along z is no hole; per section it is
    b = np.full((3, 7, 7), 4, np.uint64)
    b[:, 3, 3] = 0
    assert (R.fill_holes(b)[:, 3, 3] == 0).all()
    assert (R.apply_block(b, "fill_holes", xy=True)[:, 3, 3] == 4).all()
    # a hole inside a hole: both decided on the input
    c = np.full((23, 23), 4, np.uint64)
    c[2:21, 2:21] = 8            # 76 faces against 4, 4 against the hole: 76 / 80 is the boundary
    c[11, 11] = 0
    f = R.fill_holes(c)
    want = np.full((23, 23), 4, np.uint64)
    want[11, 11] = 8             # the inner decision's id, though the square around it has gone
    assert np.array_equal(f, want)
    # ties between neighbouring ids go to the smallest (neither reaches 95 % here, so nothing changes)
    d = np.full((5, 6), 4, np.uint64)
    d[:, 3:] = 3
    d[2, 2:4] = 0
    assert np.array_equal(R.fill_holes(d), d)


def test_morph_blocks_on_ragged_shapes():
    blocks = RF.morph_blocks((5, 40, 70), (4, 16, 16), 32, 3, xy=False)
    assert blocks == [
        (((0, 4), (0, 32), (0, 32)), ((0, 5), (0, 35), (0, 35))),
        (((0, 4), (0, 32), (32, 64)), ((0, 5), (0, 35), (29, 67))),
        (((0, 4), (0, 32), (64, 70)), ((0, 5), (0, 35), (61, 70))),
        (((0, 4), (32, 40), (0, 32)), ((0, 5), (29, 40), (0, 35))),
        (((0, 4), (32, 40), (32, 64)), ((0, 5), (29, 40), (29, 67))),
        (((0, 4), (32, 40), (64, 70)), ((0, 5), (29, 40), (61, 70))),
        (((4, 5), (0, 32), (0, 32)), ((1, 5), (0, 35), (0, 35))),
        (((4, 5), (0, 32), (32, 64)), ((1, 5), (0, 35), (29, 67))),
        (((4, 5), (0, 32), (64, 70)), ((1, 5), (0, 35), (61, 70))),
        (((4, 5), (32, 40), (0, 32)), ((1, 5), (29, 40), (0, 35))),
        (((4, 5), (32, 40), (32, 64)), ((1, 5), (29, 40), (29, 67))),
        (((4, 5), (32, 40), (64, 70)), ((1, 5), (29, 40), (61, 70))),
    ]
    # --xy: no halo along z; the block size snaps to whole chunks (round(40 / 16) = 2, round(20 / 16) = 1, never below one)
    assert RF.morph_blocks((3, 30, 50), (2, 16, 16), 40, 5, xy=True) == [
        (((0, 2), (0, 30), (0, 32)), ((0, 2), (0, 30), (0, 37))),
        (((0, 2), (0, 30), (32, 50)), ((0, 2), (0, 30), (27, 50))),
        (((2, 3), (0, 30), (0, 32)), ((2, 3), (0, 30), (0, 37))),
        (((2, 3), (0, 30), (32, 50)), ((2, 3), (0, 30), (27, 50))),
    ]
    assert RF.morph_blocks((2, 20, 20), (2, 16, 16), 20, 0, xy=False) == [
        (((0, 2), (0, 16), (0, 16)),) * 2, (((0, 2), (0, 16), (16, 20)),) * 2,
        (((0, 2), (16, 20), (0, 16)),) * 2, (((0, 2), (16, 20), (16, 20)),) * 2]
    assert RF.morph_blocks((2, 20, 20), (2, 16, 16), 1, 0, xy=False)[0][0] == ((0, 2), (0, 16), (0, 16))
    assert len(RF.morph_blocks((2, 20, 20), (2, 16, 16), 2048, 64, xy=False)) == 1


@pytest.mark.parametrize("op,n,xy", [("dilate", 2, False), ("erode", 2, False), ("opening", 1, False), ("closing", 2, False),
                                     ("dilate", 3, True), ("erode", 1, True), ("opening", 2, True), ("closing", 1, True)])
def test_blocks_equal_the_whole_volume_when_the_context_covers_the_reach(op, n, xy):
    vol = R.cells((10, 40, 52), 25, 3)
    reach = n if op in ("dilate", "erode") else 2 * n
    whole = R.apply_block(vol, op, n, xy)
    assert np.array_equal(R.morph_volume(vol, (4, 8, 8), op, n, xy, context=reach, block_size=16), whole)
    assert not np.array_equal(whole, vol)


def test_a_context_below_the_reach_shows_at_the_seams():
    vol = R.cells((10, 40, 52), 25, 3)
    assert not np.array_equal(R.morph_volume(vol, (4, 8, 8), "erode", 2, False, context=0, block_size=16), R.apply_block(vol, "erode", 2))


def test_command_line(tmp_path):
    assert "morph" in RF.refine.commands
    cmd = RF.refine.commands["morph"]
    opts = {p.name: p for p in cmd.params}
    assert tuple(opts["op"].type.choices) == RF.MORPH_OPS == ("dilate", "erode", "opening", "closing", "fill_holes")
    assert sorted(opts["iterations"].opts) == ["--iterations", "-n"]   # -n is --iterations here, as in the reference
    assert sorted(opts["context"].opts) == ["--context", "-c"] and sorted(opts["block_size"].opts) == ["--block_size", "-b"]
    assert sorted(opts["num_workers"].opts) == ["--num_workers", "-w"]
    assert (opts["iterations"].default, opts["context"].default, opts["block_size"].default, opts["num_workers"].default) == (1, 64, 2048, 20)
    assert opts["op"].required and opts["xy"].is_flag
    assert RF.MERGE_THRESHOLD == (19, 20) == R.MERGE_THRESHOLD
    for op in RF.MORPH_OPS:
        assert RF.derived_dataset("/data/a.zarr/seg", op) == f"/data/a.zarr/seg_{op}"
    from bootstrapper_amd.cli import cli
    res = CliRunner().invoke(cli, ["refine", "morph", "--help"])
    assert res.exit_code == 0, res.output
    for word in ("--op", "--iterations", "-n", "--xy", "--context", "--block_size", "--num_workers", "2*iterations", "fill_holes"):
        assert word in res.output, word
    # an input outside a single .zarr has no default output name
    from bootstrapper_amd.zarr_io import prepare_ds
    loose = str(tmp_path / "a.zarr" / "b.zarr" / "seg")   # inside two containers
    prepare_ds(loose, shape=(2, 8, 8), dtype=np.uint64, chunk_shape=(2, 8, 8))
    res = CliRunner().invoke(cli, ["refine", "morph", "-i", loose, "--op", "erode"])
    assert res.exit_code == 1 and "give --out_array" in res.output
    with pytest.raises(Exception, match="give --out_array"):
        RF.morph(loose, op="erode")
