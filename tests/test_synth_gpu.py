"""csrc/synth.hip against tests/synth_ref.py: bit-equal, except the float32 gaussian, which is held to scipy's float64 result
by a gate derived from its tap count.  Generated volumes of 12 x 40 x 44 (depth below the gaussian's radius, width no
multiple of 32), 9 x 33 x 65 (three words per row, one of them a single bit) and a single section."""
import random

import numpy as np
import pytest
import torch

import synth_ref as R
from bootstrapper_amd import synth_labels as S

pytestmark = pytest.mark.gpu

SHAPES = [(12, 40, 44), (9, 33, 65), (1, 40, 44)]
STRUCTS = {"star": S.star(5), "disk": S.disk(3), "ellipse": S.ellipse(4, 2), "cross": S.binary_structure(1)}


@pytest.fixture(scope="module")
def engines():
    """engines(shape): an engine made for exactly that shape, so that an index past the case's extent leaves the workspace (and, under
    tests/test_redzones_gpu.py, lands in a guard zone); one per shape for the whole module"""
    made = {}

    def get(shape):
        shape = tuple(int(v) for v in shape)
        if shape not in made:
            made[shape] = S.SynthEngine(shape, 0)
        return made[shape]
    yield get
    for e in made.values():
        e.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def border_points(shape, seed):
    d, h, w = shape
    rng = np.random.default_rng(seed)
    pts = [[0, 0, 0], [d - 1, h - 1, w - 1], [0, 0, w - 1], [d // 2, h - 1, 0], [d // 2, h // 2, 31 % w], [d // 2, 3, 32 % w]]
    pts += [[int(rng.integers(d)), int(rng.integers(h)), int(rng.integers(w))] for _ in range(6)]
    return np.array(pts, dtype=np.int32)


def blocks(shape, holes=True):
    """labelled boxes of 11 x 9 with a few background voxels; the ids change every 5 sections"""
    d, h, w = shape
    z, y, x = np.indices(shape)
    lab = (z // 5) * 50 + (y // 11) * 8 + x // 9 + 1
    if holes:
        lab[(y + 2 * x + z) % 17 == 0] = 0
    return lab.astype(np.int64)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", sorted(STRUCTS))
@pytest.mark.parametrize("iterations", [1, 10])
def test_dilation(engines, shape, kind, iterations):
    eng = engines(shape)
    pts = border_points(shape, 3)
    idx, its = np.zeros(shape[0], dtype=np.int32), np.full(shape[0], iterations, dtype=np.int32)
    got = host(eng.dilate_points(shape, pts, [STRUCTS[kind]], idx, its))
    assert np.array_equal(got, R.dilate_points(shape, pts, [STRUCTS[kind]], idx, its))


def test_dilation_per_section_tables_and_refusal(engines):
    eng = engines((9, 33, 65))
    shape = (9, 33, 65)
    pts = border_points(shape, 4)
    structs = list(STRUCTS.values())
    idx = (np.arange(9) % 4).astype(np.int32)
    its = np.array([1, 2, 3, 10, 5, 1, 7, 2, 0], dtype=np.int32)
    assert np.array_equal(host(eng.dilate_points(shape, pts, structs, idx, its)), R.dilate_points(shape, pts, structs, idx, its))
    # two bit planes of 1100 rows of 10 words are 88,000 bytes: refused, not mis-computed
    big = S.SynthEngine((1, 1100, 300), 0)
    with pytest.raises(S._lib.BsmiError, match="LDS") as e:
        big.dilate_points((1, 1100, 300), pts[:1] * 0, structs, idx[:1], its[:1])
    assert e.value.code == S._lib.ERR_INVALID
    big.close()
    with pytest.raises(S._lib.BsmiError):
        eng.dilate_points(shape, np.array([[0, 33, 0]], dtype=np.int32), structs, idx, its)


@pytest.fixture(scope="module")
def tube_cases():
    """(foreground, reference labelling, count, reference expansion, reference result) per case, computed once"""
    cases = {}
    # a drawn plan: (6, 40, 44) at the first seed whose plan is tubes at anisotropy 2 -> 12 x 40 x 44
    seed = next(s for s in range(200) if (lambda p: p.choice == "tubes" and p.anisotropy == 2)(S.draw_plan(random.Random(s), (6, 40, 44), (2, 4))))
    p = S.draw_plan(random.Random(seed), (6, 40, 44), (2, 4))
    cases["plan"] = R.dilate_points(p.generated_shape, p.points, p.structs, p.struct_index, p.dilations)
    # tubes in one corner of 9 x 33 x 65: the voxels beyond x = 30 are farther than the depth and take max + 1
    pts = np.array([[1, 3, 2], [4, 9, 6], [7, 20, 3], [8, 30, 12], [4, 15, 9]], dtype=np.int32)
    cases["far"] = R.dilate_points((9, 33, 65), pts, [S.binary_structure(2)], np.zeros(9, dtype=np.int32), np.full(9, 2, dtype=np.int32))
    one = np.zeros((1, 40, 44), dtype=np.int32)
    one[0, 5:9, 5:9] = one[0, 20, 30:41] = one[0, 9, 9] = one[0, 39, 0] = 1
    cases["section"] = one
    out = {}
    for name, fg in cases.items():
        lab, n = R.label(fg)
        ex = R.expand(lab, fg.shape[0], n + 1)
        out[name] = (fg, lab, n, ex, R.label(ex))
    assert (out["far"][3] == out["far"][2] + 1).any() and not (out["plan"][3] == out["plan"][2] + 1).all()
    return out


@pytest.mark.parametrize("name", ["plan", "far", "section"])
def test_tubes_branch(engines, tube_cases, name):
    fg, lab, n, ex, (final, m) = tube_cases[name]
    eng = engines(fg.shape)
    got, gn = eng.label(dev(fg))
    assert gn == n and np.array_equal(host(got), lab)
    assert np.array_equal(host(eng.expand(dev(lab), fg.shape[0], n + 1)), ex)
    got, gm = eng.tubes(dev(fg))
    assert gm == m and np.array_equal(host(got), final)


def test_expand_tie_rule(engines):
    """features at equal distances along every axis and diagonally: the lowest raster index wins"""
    eng = engines((5, 9, 9))
    lab = np.zeros((5, 9, 9), dtype=np.int32)
    for k, (z, y, x) in enumerate([(2, 4, 0), (2, 4, 8), (2, 0, 4), (2, 8, 4), (0, 4, 4), (4, 4, 4), (0, 0, 0), (4, 8, 8)]):
        lab[z, y, x] = k + 1
    want = R.expand(lab, 2, 99)
    assert want[2, 4, 4] == 5 and (want == 99).any()        # centre: two features at distance 2, four at 4; (0, 4, 4) comes first
    assert np.array_equal(host(eng.expand(dev(lab), 2, 99)), want)
    assert np.array_equal(host(eng.expand(dev(lab), 5, 99)), R.expand(lab, 5, 99))


@pytest.mark.parametrize("shape", SHAPES)
def test_gaussian_against_float64(engines, shape):
    eng = engines(shape)
    g = torch.Generator(device="cuda").manual_seed(5)
    noise = torch.rand(shape, generator=g, dtype=torch.float32, device="cuda")
    got = host(eng.gaussian(noise)).astype(np.float64)
    err = np.abs(got - R.gaussian(host(noise))).max()
    print(f"gaussian {shape}: max abs err {err:.3e}, gate {R.gaussian_gate():.3e}")
    assert err <= R.gaussian_gate()


def plateau_field(shape):
    rng = np.random.default_rng(11)
    return rng.integers(0, 5, shape).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["blurred", "plateaus"])
def test_argmax_filter_and_basins(engines, shape, kind):
    eng = engines(shape)
    if kind == "blurred":       # the device's own field, read back: what the random branch sees
        g = torch.Generator(device="cuda").manual_seed(6)
        fld = eng.gaussian(torch.rand(shape, generator=g, dtype=torch.float32, device="cuda"))
    else:
        fld = dev(plateau_field(shape))
    f = host(fld)
    pos = eng.argmax_filter(fld, S.PEAK_WINDOW)
    want_pos = R.argmax_filter(f, S.PEAK_WINDOW)
    assert np.array_equal(host(pos), want_pos)
    lab, n = eng.basins(fld, pos)
    want, m = R.basins(f, want_pos)
    assert n == m and np.array_equal(host(lab), want)
    if kind == "plateaus":
        assert (f.ravel()[want_pos] == f).sum() > m            # voxels tied with their window's maximum that are no roots


def test_random_branch(engines):
    eng = engines((12, 40, 44))
    g = torch.Generator(device="cuda").manual_seed(8)
    noise = torch.rand((12, 40, 44), generator=g, dtype=torch.float32, device="cuda")
    f = host(eng.gaussian(noise))
    assert np.array_equal(host(eng.random_labels(noise)), R.basins(f, R.argmax_filter(f, S.PEAK_WINDOW))[0])


def test_argmax_filter_even_window_and_mask(engines):
    eng = engines((9, 33, 65))
    f = plateau_field((9, 33, 65))
    mask = (blocks((9, 33, 65)) % 3 != 0).astype(np.uint8)
    f *= mask
    pos = eng.argmax_filter(dev(f), 22)
    assert np.array_equal(host(pos), R.argmax_filter(f, 22))
    lab, n = eng.basins(dev(f), pos, dev(mask))
    want, m = R.basins(f, host(pos), mask)
    assert n == m and np.array_equal(host(lab), want) and ((want == 0) == (mask == 0)).all()


@pytest.mark.parametrize("anisotropy", [2, 5, 13])
@pytest.mark.parametrize("drop3,drop5", [(False, False), (True, False), (True, True)])
def test_finish(engines, anisotropy, drop3, drop5):
    eng = engines((12, 40, 44))
    lab = (blocks((12, 40, 44)) % 31).astype(np.int32)
    got = eng.finish(dev(lab), drop3, drop5, anisotropy)
    want = R.finish(lab, drop3, drop5, anisotropy)
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape == ((-(-12 // anisotropy) if anisotropy <= 12 else 1), 40, 44)
    assert np.array_equal(host(got), want)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("max_steps", [1, 3])
def test_grow_boundary(engines, shape, max_steps):
    eng = engines(shape)
    lab = blocks(shape)                    # its boxes touch every face of every section
    want = R.grow_boundary(lab, 1234567, max_steps)
    assert np.array_equal(host(eng.grow_boundary(dev(lab), 1234567, max_steps)), want)
    assert (want[:, 0, :] != 0).any() and (want != lab).any()
    steps = {S.grow_steps(1234567, z, int(v), max_steps) for z in range(shape[0]) for v in np.unique(lab[z]) if v}
    assert steps == set(range(max_steps + 1)) or shape[0] == 1


def dumbbell():
    """label 7: two balls of radius 9 joined by a thin bar, in sections 1..7 of 9; label 3 elsewhere in section 0"""
    lab = np.zeros((9, 33, 65), dtype=np.int64)
    z, y, x = np.indices(lab.shape)
    for cx in (14, 48):
        lab[((z - 4) * 3) ** 2 + (y - 16) ** 2 + (x - cx) ** 2 <= 81] = 7
    lab[4, 15:18, 14:48] = 7
    lab[0, 2:6, 2:30] = 3
    lab[8, 20:30, 50:60] = 12
    return lab


def test_merge_stamp_present(engines):
    eng = engines((9, 33, 65))
    lab = blocks((9, 33, 65))
    t = dev(lab)
    assert eng.present(t) == [int(v) for v in np.unique(lab) if v]
    eng.merge(t, [6, 1], 2, 3)
    want = R.merge(lab, [6, 1], 2, 3)
    eng.merge(t, [8], 111, 110)
    want = R.merge(want, [8], 111, 110)
    assert np.array_equal(host(t), want)
    for k, (z, y, x, s) in enumerate([(0, 0, 0, S.star(8)), (8, 33 - 17, 65 - 17, S.disk(8)), (3, 5, 40, S.ellipse(8, 2)), (3, 30, 62, S.binary_structure(1))]):
        eng.stamp(t, z, y, x, s, 500 + k)
        want = R.stamp(want, z, y, x, s, 500 + k)
    assert np.array_equal(host(t), want)
    assert eng.present(t) == [int(v) for v in np.unique(want) if v]
    with pytest.raises(S._lib.BsmiError):
        eng.stamp(t, 0, 33 - 16, 0, S.disk(8), 1)


@pytest.mark.parametrize("window,sections", [(15, [4, 2]), (15, [0]), (50, [4]), (22, [8, 4])])
def test_split(engines, window, sections):
    eng = engines((9, 33, 65))
    lab = dumbbell()
    scale = int(lab.max())
    want, m = R.split(lab, 7, window, sections, scale)
    t = dev(lab)
    n = eng.split(t, 7, window, sections, scale)
    assert n == m and np.array_equal(host(t), want)
    if window == 15:
        assert m >= 2
    if sections == [0]:                      # label 7 has no voxel in section 0: nothing changes
        assert np.array_equal(want, lab)
    elif m >= 2:                             # the reference's quirk: fragment 1 takes the current maximum, an id in use
        assert (want[4][lab[4] == 7] == 12).any() and (want[4][lab[4] == 7] == 24).any()


def test_obfuscate_follows_the_operation_list(engines):
    """the whole node with every operation likely: the same draws and the same labels as the restatement"""
    eng = engines((9, 33, 65))
    lab = dumbbell() + blocks((9, 33, 65), holes=False) * (dumbbell() == 0)
    for seed in (1, 2, 3):
        got = eng.obfuscate(dev(lab), random.Random(seed), p_split=0.7, p_merge=0.7, p_artifact=0.7)
        want = R.obfuscate(lab, random.Random(seed), p_split=0.7, p_merge=0.7, p_artifact=0.7)
        assert np.array_equal(host(got), want)
        assert (want != lab).any()
    assert np.array_equal(host(eng.obfuscate(dev(lab * 0), random.Random(1))), lab * 0)
