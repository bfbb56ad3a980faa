"""`bs utils` without a device: the argument the raw-mask driver rests on (the reference's block-by-block double closing equals one
closing of the zero-extended section), the pyramid planning, the name rules, the command line's refusals and the merge table."""
import json
import os

import click
import numpy as np
import pytest

import utils_ref as R

OFFSET, VOXEL = (40, 4, 12), (40, 4, 4)


def _raw(shape, seed, density=0.02):
    rng = np.random.default_rng(seed)
    return ((rng.random(shape) < density) * rng.integers(1, 256, shape)).astype(np.uint8)


@pytest.mark.parametrize("shape,chunks", [((3, 70, 101), (2, 32, 32)), ((2, 45, 130), (1, 16, 64)), ((2, 97, 64), (2, 40, 24)),
                                          ((1, 21, 23), (1, 8, 8))])
def test_blockwise_double_closing_is_one_closing_of_the_zero_extended_section(shape, chunks):
    raw = _raw(shape, sum(shape))
    raw[:, 0, 0] = raw[:, -1, -1] = 9
    want = R.mask_blockwise(raw, chunks)
    assert np.array_equal(R.closing_volume(raw), want)
    assert 0 < want.mean() < 1 and not np.array_equal(want, raw != 0)


def test_disk_is_the_one_of_the_issue():
    d = R.disk(10)
    assert d.shape == (21, 21) and int(d.sum()) == 317
    assert [int(r.sum() - 1) // 2 for r in d] == [0, 4, 6, 7, 8, 8, 9, 9, 9, 9, 10, 9, 9, 9, 9, 8, 8, 7, 6, 4, 0]


def test_pyramid_plan_down_snaps_the_roi_outwards():
    from bootstrapper_amd.utils import pyramid_plan
    p = pyramid_plan("/x/vol.zarr/raw", (5, 70, 101), OFFSET, VOXEL, [(1, 2, 2), (2, 2, 2)], "down")
    assert p["name"] == "raw" and p["base"] == "/x/vol.zarr/raw" and p["start"] == "/x/vol.zarr/raw/s0"
    assert p["renames"] == [("/x/vol.zarr/raw", "/x/vol.zarr/raw__tmp"), ("/x/vol.zarr/raw__tmp", "/x/vol.zarr/raw/s0")]
    s1, s2 = p["levels"]
    assert (s1["name"], s1["path"], s1["factor"]) == ("s1", "/x/vol.zarr/raw/s1", (1, 2, 2))
    assert s1["voxel_size"] == (40, 8, 8) and s1["offset"] == (40, 0, 8)    # y snaps 4 -> 0, x 12 -> 8
    assert s1["lead"] == (0, 1, 1) and s1["shape"] == (5, 36, 51)           # ends 240, 284 -> 288, 416
    assert (s2["name"], s2["factor"]) == ("s2", (2, 2, 2))
    assert s2["voxel_size"] == (80, 16, 16) and s2["offset"] == (0, 0, 0)
    assert s2["lead"] == (1, 0, 1) and s2["shape"] == (3, 18, 26)


def test_pyramid_plan_up_counts_down_to_s0():
    from bootstrapper_amd.utils import pyramid_plan
    p = pyramid_plan("/x/vol.zarr/labels", (5, 70, 101), OFFSET, VOXEL, [(1, 2, 2), (2, 2, 2)], "up")
    assert p["start"] == "/x/vol.zarr/labels/s2" and [lv["name"] for lv in p["levels"]] == ["s1", "s0"]
    assert [lv["voxel_size"] for lv in p["levels"]] == [(40, 2, 2), (20, 1, 1)]
    assert [lv["shape"] for lv in p["levels"]] == [(5, 140, 202), (10, 280, 404)]
    assert all(lv["offset"] == OFFSET and lv["lead"] == (0, 0, 0) for lv in p["levels"])
    with pytest.raises(click.ClickException, match="divisible"):
        pyramid_plan("/x/vol.zarr/labels", (5, 70, 101), OFFSET, VOXEL, [(3, 1, 1)], "up")


def test_pyramid_plan_continues_from_a_level():
    from bootstrapper_amd.utils import pyramid_plan
    p = pyramid_plan("/x/vol.zarr/raw/s2", (5, 70, 101), OFFSET, VOXEL, [(2, 2, 2)], "down")
    assert p["name"] == "raw" and p["base"] == "/x/vol.zarr/raw" and p["renames"] == [] and p["start"] == "/x/vol.zarr/raw/s2"
    assert [lv["name"] for lv in p["levels"]] == ["s3"]
    p = pyramid_plan("/x/vol.zarr/raw/s2", (5, 70, 101), OFFSET, VOXEL, [(1, 2, 2)], "up")
    assert p["renames"] == [] and [lv["path"] for lv in p["levels"]] == ["/x/vol.zarr/raw/s1"]
    # no room below s1 for two levels: the input becomes the new top
    p = pyramid_plan("/x/vol.zarr/labels/s1", (5, 70, 101), OFFSET, VOXEL, [(1, 2, 2), (1, 2, 2)], "up")
    assert p["renames"] == [("/x/vol.zarr/labels/s1", "/x/vol.zarr/labels/s2")] and p["start"] == "/x/vol.zarr/labels/s2"
    assert [lv["name"] for lv in p["levels"]] == ["s1", "s0"] and p["name"] == "labels"


def test_pyramid_plan_refuses_a_wrong_count_of_values():
    from bootstrapper_amd.utils import pyramid_plan
    with pytest.raises(click.ClickException, match="2 values"):
        pyramid_plan("/x/vol.zarr/raw", (5, 70, 101), OFFSET, VOXEL, [(2, 2)], "down")


def test_label_names_and_factors():
    from bootstrapper_amd.utils import is_label_array, parse_factor
    assert is_label_array("raw", np.uint64) and is_label_array("raw", np.dtype("<u4"))
    assert not is_label_array("raw", np.uint8) and not is_label_array("volumes/image", np.uint16)
    for name in ("labels", "gt_lbl", "frag_IDs", "raw_mask", "a/b/Seg_01"):
        assert is_label_array(name, np.uint8), name
    assert not is_label_array("labels/raw", np.uint8)   # the last path component decides
    assert parse_factor("2,2,2") == (2, 2, 2) and parse_factor("1 2 2") == (1, 2, 2) and parse_factor("1, 2,4") == (1, 2, 4)
    with pytest.raises(ValueError):
        parse_factor("2,x")


def test_merge_table_takes_the_first_key_in_file_order():
    from bootstrapper_amd.utils import merge_mapping
    luts = json.loads('{"merges": {"9": [1, 4], "2": [1, 3], "18446744073709551615": [4, 7]}}')
    keys, vals = merge_mapping(luts)
    assert keys.dtype == np.uint64 and vals.dtype == np.uint64
    assert dict(zip(keys.tolist(), vals.tolist())) == {1: 9, 4: 9, 3: 2, 7: (1 << 64) - 1}
    a = np.array([[[0, 1, 2, 3, 4, 7, 9]]], np.uint32)
    assert R.merge(a, luts["merges"]).tolist() == [[[0, 9, 2, 2, 9, (1 << 64) - 1, 9]]]


def test_mask_tiles_cover_the_volume_with_a_clipped_halo():
    from bootstrapper_amd.utils import mask_tiles
    tiles = mask_tiles((5, 70, 101), (2, 32, 32), (32, 70), 20)
    seen = np.zeros((5, 70, 101), np.int32)
    for write, read in tiles:
        seen[tuple(slice(lo, hi) for lo, hi in write)] += 1
        assert read[0] == write[0]
        for (wl, wh), (rl, rh), n in zip(write[1:], read[1:], (70, 101)):
            assert rl == max(0, wl - 20) and rh == min(n, wh + 20)
    assert (seen == 1).all() and len(tiles) == 3 * 3 * 2   # rows of 32, columns of 64 (whole chunks)


# ---- command line ----

def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


@pytest.fixture()
def store(tmp_path):
    from bootstrapper_amd.zarr_io import prepare_ds
    root = str(tmp_path / "vol.zarr")
    keep = dict(offset=OFFSET, voxel_size=VOXEL, chunk_shape=(2, 32, 32), axis_names=["z", "y", "x"], units=["nm"] * 3)
    prepare_ds(root + "/raw", (5, 70, 101), dtype=np.uint8, **keep)[:] = _raw((5, 70, 101), 1)
    for level in ("s0", "s1"):
        prepare_ds(f"{root}/pyr/{level}", (5, 70, 101), dtype=np.uint8, **keep)[:] = 1
    return root


def _run(*args):
    from click.testing import CliRunner
    from bootstrapper_amd.cli import cli
    return CliRunner().invoke(cli, list(args))


def test_help_lists_the_commands():
    res = _run("utils", "--help")
    assert res.exit_code == 0, res.output
    for name in ("mask", "scale_pyramid", "bbox", "merge"):
        assert name in res.output
    for name in ("convert", "download"):
        assert name not in res.output
    res = _run("utils", "scale_pyramid", "--help")
    for opt in ("--in_array", "--scales", "--chunk_shape", "--mode"):
        assert opt in res.output
    assert "--padding" in _run("utils", "bbox", "--help").output and "--luts" in _run("utils", "merge", "--help").output


def test_wrong_scale_count_and_existing_level_are_refused(store):
    from bootstrapper_amd.utils import scale_pyramid
    before = _tree(store)
    with pytest.raises(click.ClickException, match="2 values"):
        scale_pyramid(store + "/raw", ["2,2"], mode="down")
    with pytest.raises(click.ClickException, match="already exists"):
        scale_pyramid(store + "/pyr/s0", ["1,2,2"], mode="down")
    with pytest.raises(click.ClickException, match="3 spatial dimensions"):
        scale_pyramid(store + "/raw", ["2,2,2"], chunk_shape="8,8", mode="down")
    res = _run("utils", "scale_pyramid", "-i", store + "/raw", "-s", "2,2", "-m", "down")
    assert res.exit_code == 1 and "Error:" in res.output and "2 values" in res.output
    res = _run("utils", "scale_pyramid", "-i", store + "/pyr/s0", "-s", "1,2,2", "-m", "down")
    assert res.exit_code == 1 and "already exists" in res.output
    assert _tree(store) == before


def test_upscaling_an_image_is_refused_before_anything_is_touched(store):
    before = _tree(store)
    res = _run("utils", "scale_pyramid", "-i", store + "/raw", "-s", "1,2,2", "-m", "up")
    assert isinstance(res.exception, NotImplementedError) and "upscaling an image" in str(res.exception)
    assert _tree(store) == before and not os.path.exists(store + "/raw/s1")
