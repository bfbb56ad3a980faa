"""Host side of the synthetic-label source: the draw plan, the operation list, the structuring bitmaps, the numpy
restatement (tests/synth_ref.py) against scipy where scipy has no choice to make, and the opt-in routing.  No GPU."""
import random

import numpy as np
import pytest
from scipy import ndimage

import synth_ref as R
from bootstrapper_amd import synth_labels as S


def _plan_key(p):
    return (p.anisotropy, p.choice, p.radii, None if p.points is None else p.points.tobytes(),
            None if p.dilations is None else p.dilations.tobytes(), None if p.struct_index is None else p.struct_index.tobytes(),
            p.noise_seed, p.drop3, p.drop5)


def test_plan_is_reproducible_per_seed_and_differs_between_seeds():
    a = [S.draw_plan(random.Random(s), (24, 148, 148), (2, 10)) for s in (42, 42, 43)]
    assert _plan_key(a[0]) == _plan_key(a[1]) != _plan_key(a[2])
    # both branches occur, and a tubes plan holds what the reference draws: 5..5a points inside [1, n - 1], 1..10 dilations
    seen = set()
    for seed in range(40):
        p = S.draw_plan(random.Random(seed), (6, 40, 44), S.anisotropy_range((40, 4, 4)))
        seen.add(p.choice)
        assert 2 <= p.anisotropy <= 10 and p.generated_shape == (6 * p.anisotropy, 40, 44) and len(p.structs) == 7
        if p.choice == "tubes":
            assert 5 <= len(p.points) <= 5 * p.anisotropy and p.points.min() >= 1
            assert (p.points < np.array(p.generated_shape)).all()
            assert len(p.dilations) == p.generated_shape[0] and p.dilations.min() >= 1 and p.dilations.max() <= 10
            assert p.struct_index.min() >= 0 and p.struct_index.max() < 7
    assert seen == {"tubes", "random"}
    assert S.anisotropy_range((40, 4, 4)) == (2, 10) and S.anisotropy_range((8, 8, 8)) == (2, 4)


def test_operation_list_follows_the_single_r_rule():
    class Fixed:
        def __init__(self, vals):
            self.vals = list(vals)

        def random(self):
            return self.vals.pop(0)

    # one r per try against all three probabilities: r below all gives all three in the reference's order
    assert S.draw_operations(Fixed([0.05, 0.5, 0.15, 0.25, 0.95]), 5, 0.1, 0.2, 0.3) == ["split", "merge", "artifact", "merge", "artifact", "artifact"]
    rng = random.Random(7)
    ops = S.draw_operations(rng)
    same = random.Random(7)
    assert rng.random() == [same.random() for _ in range(6)][5]    # five draws, no more
    assert len(ops) % 3 == 0                                                   # equal probabilities: all three or none


@pytest.mark.parametrize("make,extent", [(lambda r: S.star(r), lambda r: (2 * r + 1 + 2 * (r // 2),) * 2),
                                          (lambda r: S.disk(r), lambda r: (2 * r + 1,) * 2)])
def test_star_and_disk(make, extent):
    for r in range(1, 9):
        b = make(r)
        assert b.shape == extent(r) and max(b.shape) <= 32
        assert np.array_equal(b, b[::-1]) and np.array_equal(b, b[:, ::-1]) and np.array_equal(b, b.T)
        assert b[b.shape[0] // 2].all() and b[:, b.shape[1] // 2].all()       # reaches its extent along both axes
        rows, h, w = S.pack_bitmap(b)
        assert (h, w) == b.shape and all(((int(rows[i]) >> j) & 1) == int(b[i, j]) for i in range(h) for j in range(w))
    # star(2): the 5 x 5 square and the four tips of the diamond beyond it; disk(1): the cross
    assert S.star(1).all() and S.star(2).sum() == 25 + 4 and S.disk(1).sum() == 5


def test_ellipse_and_binary_structure():
    for w in range(2, 9):
        for h in range(2, 9):
            b = S.ellipse(w, h)
            assert b.shape == (2 * h + 1, 2 * w + 1)
            assert np.array_equal(b, b[::-1]) and np.array_equal(b, b[:, ::-1])
            assert b[h].all() and b[:, w].all()
    assert not S.ellipse(8, 8)[0, 0] and not S.ellipse(2, 8)[0, 0]       # (8 / 9)^2 + (2 / 3)^2 > 1
    assert np.array_equal(S.binary_structure(1), ndimage.generate_binary_structure(2, 1))
    assert np.array_equal(S.binary_structure(2), ndimage.generate_binary_structure(2, 2))
    with pytest.raises(ValueError):
        S.pack_bitmap(np.ones((33, 3), dtype=bool))


def test_ref_dilation_is_scipys():
    rng = np.random.default_rng(0)
    sec = rng.random((21, 37)) < 0.02
    sec[0, 0] = sec[20, 36] = sec[0, 17] = True
    lop = np.zeros((5, 7), dtype=bool)      # no symmetry at all: the origin and the direction of the shift matter
    lop[0, 1] = lop[2, 3] = lop[4, 6] = lop[3, 0] = True
    for struct in (S.star(3), S.disk(2), S.ellipse(4, 2), S.binary_structure(1), lop):
        for it in (1, 3):
            assert np.array_equal(R.dilate_section(sec, struct, it), ndimage.binary_dilation(sec, structure=struct, iterations=it))


def test_ref_feature_transform_and_labelling_against_scipy():
    rng = np.random.default_rng(1)
    fg = rng.random((7, 19, 23)) < 0.01
    fg[3, 4:9, 5] = True
    d2, idx = R.nearest_feature(fg)
    dist = ndimage.distance_transform_edt(~fg)
    assert np.array_equal(d2, np.rint(dist ** 2).astype(np.int64))
    zz, yy, xx = np.unravel_index(idx, fg.shape)
    gz, gy, gx = np.indices(fg.shape)
    assert fg[zz, yy, xx].all() and np.array_equal((zz - gz) ** 2 + (yy - gy) ** 2 + (xx - gx) ** 2, d2)
    # the tie rule: two features at one distance, the lower raster index is taken
    two = np.zeros((1, 1, 5), dtype=bool)
    two[0, 0, 0] = two[0, 0, 4] = True
    assert R.nearest_feature(two)[1].ravel().tolist() == [0, 0, 0, 4, 4]
    binary = rng.random((6, 15, 17)) < 0.2
    lab, n = R.label(binary.astype(np.int32))
    want, m = ndimage.label(binary, structure=np.ones((3, 3, 3), dtype=bool))
    assert n == m and np.array_equal(lab, want)       # scipy numbers components by their first voxel in raster order too
    # equal values only: two touching regions of different value stay apart
    v = np.zeros((1, 3, 4), dtype=np.int32)
    v[0, :, :2], v[0, :, 2:] = 5, 2
    assert np.array_equal(R.label(v)[0][0, 0], [1, 1, 2, 2])


def test_ref_argmax_filter_forms_agree_and_follow_scipy():
    rng = np.random.default_rng(2)
    f = rng.integers(0, 4, (3, 6, 7)).astype(np.float32)       # plateaus; depth below the window: repeated reflection
    for w in (4, 5, 9):
        pos = R.argmax_filter(f, w)
        assert np.array_equal(pos, R.argmax_filter_brute(f, w))
        assert np.array_equal(f.ravel()[pos], ndimage.maximum_filter(f, size=w, mode="reflect"))
    lab, n = R.basins(f, R.argmax_filter(f, 5))
    assert lab.min() >= 1 and lab.max() == n and len(np.unique(lab)) == n


def test_ref_grow_boundary_is_an_l1_ball_test():
    lab = np.zeros((2, 9, 9), dtype=np.int64)
    lab[:, :, :5], lab[:, :, 5:] = 3, 4
    seed = next(s for s in range(100) if S.grow_steps(s, 0, 3, 2) == 2 and S.grow_steps(s, 0, 4, 2) == 0)
    out = R.grow_boundary(lab, seed, 2)
    assert (out[0][:, :3] == 3).all() and (out[0][:, 3:5] == 0).all() and (out[0][:, 5:] == 4).all()   # the border does not erode
    assert {S.grow_steps(s, 1, 3, 2) for s in range(64)} == {0, 1, 2}


def test_make_sample_source_routes_on_the_opt_in():
    from bootstrapper_amd.train import SyntheticSource, make_sample_source
    nc = {"input_shape": [24, 148, 148], "output_shape": [4, 56, 56],
          "inputs": {"2d_lsds": {"dims": 6, "sigma": 10, "downsample": 2, "grow_boundary": 1},
                     "2d_affs": {"dims": 6, "neighborhood": [[-1, 0], [0, -1], [-9, 0], [0, -9], [-27, 0], [0, -27]], "grow_boundary": 1}},
          "outputs": {"3d_affs": {"dims": 3, "neighborhood": [[-1, 0, 0], [0, -1, 0], [0, 0, -1]], "grow_boundary": 0}}}
    with pytest.raises(NotImplementedError, match="3d_affs_from_2d_mtlsd.*synthetic_labels"):
        make_sample_source({"voxel_size": [40, 4, 4]}, nc, 0, 0)
    src = make_sample_source({"voxel_size": [40, 4, 4], "synthetic_labels": True}, nc, 0, 3)     # no `samples`, no GPU touched
    assert isinstance(src, SyntheticSource) and src.engine is None
    assert src.aniso == (2, 10) and src.in_grow == 1 and src.out_grow == 0 and [k for k, _ in src.inputs] == ["2d_lsds", "2d_affs"]
    assert src.rng.random() == random.Random(45).random()
    with pytest.raises(NotImplementedError):
        SyntheticSource(dict(nc, inputs={"2d_lsds": {}, "3d_lsds": {}}))
