"""The fixtures and gates of the training-target tests, before a GPU is involved (tests/targets_cases.py): two independent
restatements of the descriptors agree on every fixture, every fixture has the property it was built for, and every fault a
target kernel could have, restated on the reference, is refused by the gate the device results are held to."""
import numpy as np
import pytest

import targets_cases as TC

LSD_CASES = [(3, n) for n in TC.LSD3D_NAMES] + [(2, n) for n in TC.LSD2D_NAMES]
LSD_IDS = [f"{nd}d-{n}" for nd, n in LSD_CASES]

# 10 x the largest difference seen between the scipy restatements (after their float32 cast) and the direct sum
REFS_AGREE = 10 * 3.0e-8


@pytest.mark.parametrize("nd,name", LSD_CASES, ids=LSD_IDS)
def test_scipy_restatement_agrees_with_direct_sum(nd, name):
    """oracle/lsd_ref.py (3-D) and tests/lsd2d_ref.py (2-D) against tests/lsd_direct_ref.py on every LSD fixture.  The scipy
    restatements filter axis by axis in absolute float64 coordinates and return float32; the direct sum is float64 relative
    to the cell.  Largest difference measured over all fixtures and channels: 2.98e-8, which is the float32 cast alone (half
    a float32 step below 1.0); before the cast the two differ by 1e-13 or less.  The gate is 10 x the measured value."""
    c = TC.lsd_case(nd, name)
    ref, w = TC.lsd_reference(nd, name)
    direct = TC.lsd_direct_reference(nd, name)
    assert ref.shape == direct.shape and ref.dtype == np.float32
    err = np.abs(ref.astype(np.float64) - direct).max(axis=tuple(range(1, ref.ndim)))
    print(f"{nd}d-{name}: largest difference per channel", err)
    assert err.max() < REFS_AGREE, err
    lab = c.labels[c.roi]
    want_w = (lab != 0) if c.unl is None else (lab != 0) & (c.unl[c.roi] > 0)
    assert all(np.array_equal(w[ch], want_w.astype(np.float32)) for ch in range(w.shape[0]))
    TC.gate_lsd(direct.astype(np.float32), w, ref, w, lab)           # the gate passes what is right


@pytest.mark.parametrize("nd", [3, 2])
@pytest.mark.parametrize("name", ["thin_origin", "thin_offset", "none"])
def test_thin_fixtures_hold_labels_without_a_tap(nd, name):
    c = TC.lsd_case(nd, name)
    assert c.df == 2
    ref, _ = TC.lsd_reference(nd, name)
    lab = c.labels[c.roi]
    count0 = (lab != 0) & (ref[-1] == 0)
    assert count0.sum() >= 100, count0.sum()
    sub = c.labels[(Ellipsis,) + (slice(None, None, 2),) * nd]
    thin = np.setdiff1d(np.unique(lab[count0]), [10])
    assert len(thin) >= 3 and not np.isin(sub, thin).any()            # one voxel thick at odd coordinates: never on labels[::2]
    if name == "thin_origin":                                         # and one with taps on the sub-grid, only not inside the window
        assert 10 in lab[count0] and (sub == 10).any()
    off = ref[:nd][:, count0]
    if name == "thin_origin":                                         # minus the position / sigma survives the clip near the origin
        assert ((off > 0) & (off < 0.5)).any()
    assert (off == 0).any()


@pytest.mark.parametrize("nd", [3, 2])
@pytest.mark.parametrize("name", ["df4", "df8"])
def test_coarse_fixtures_hold_cells_of_three_labels(nd, name):
    c = TC.lsd_case(nd, name)
    assert c.df == int(name[2:])
    assert TC.cells_with_labels(c, 3) >= 16
    assert (c.labels[c.roi] == 0).any()
    if nd == 2:
        cells = [s // c.df for s in c.roi_shape]
        assert sorted(cells)[0] == 16 and sorted(cells)[1] % 16 != 0


@pytest.mark.parametrize("nd", [3, 2])
def test_edge_fixture_has_no_context(nd):
    c = TC.lsd_case(nd, "edge")
    assert all(o == 0 for o in c.roi_offset) and tuple(c.roi_shape) == c.labels.shape[-nd:]


def test_rmax_fixture_is_the_largest_window():
    from lsd_direct_ref import gauss1d
    c = TC.lsd_case(2, "rmax")
    assert [gauss1d(s / (v * c.df))[0] for s, v in zip(c.sigma, c.voxel_size)] == [60, 60]
    assert c.labels.shape == (2, 152, 160) and c.roi_offset == (60, 60) and c.roi_shape == (32, 40)
    assert (16 + 120) ** 2 * 8 + (121 + 2 * 121) * 4 == 149420


@pytest.mark.parametrize("roi,name", [(False, "highbits"), (True, "highbits")])
def test_highbits_affinity_labels_collide_modulo_2_32(roi, name):
    c = TC.aff_case(roi, name)
    ids = np.unique(c.labels[c.labels != 0])
    assert len(ids) > 8 and len(np.unique(ids & 0xFFFFFFFF)) == 1 and ids.max() > 2 ** 62
    # touching objects: the grown labels differ from the labels, and some affinity across a seam is 0
    ref = TC.aff_reference(roi, name)
    assert (ref["grown"] != c.labels).any() and (ref["affs"] == 0).any() and (ref["affs"] == 1).any()


@pytest.mark.parametrize("nd", [3, 2])
def test_highbits_lsd_labels_collide_modulo_2_32(nd):
    c = TC.lsd_case(nd, "highbits")
    ids = np.unique(c.labels[c.labels != 0])
    assert len(ids) > 8 and len(np.unique(ids & 0xFFFFFFFF)) == 1 and ids.max() > 2 ** 62


def test_clip_fixtures_have_fractions_beyond_the_clip():
    assert TC.aff_reference(False, "clip_low")["frac"] == [0.0]
    assert TC.aff_reference(False, "clip_high")["frac"] == [1.0]
    ref = TC.aff_reference(False, "all_unknown")
    assert ref["frac"] == [None] and not ref["mask"].any() and not ref["weights"].any()
    frac = TC.aff_reference(True, "regimes")["frac"]
    assert frac[0] == 1.0 and frac[1] == 0.0 and frac[2] is None and 0.05 < frac[3] < 0.95
    # clipped: 1 / (2 * 0.95) where the class is everything, 1 / (2 * 0.05) would be the other class
    w = TC.aff_reference(True, "regimes")["weights"]
    assert np.allclose(w[:, 0], 1 / 1.9) and np.allclose(w[:, 1], 1 / 1.9) and not w[:, 2].any()


def test_stride_fixture_exceeds_one_pass_of_the_grid():
    c = TC.aff_case(True, "stride")
    assert int(np.prod(c.roi_shape)) > TC.GRID_CAP and c.labels.shape[0] == 2 and c.steps == 0 and len(c.nhood) == 2


def test_neighbourhood_fixtures():
    assert TC.aff_case(False, "product9").labels.shape[0] == 6 and len(TC.aff_case(False, "product9").nhood) == 9
    assert len(TC.aff_case(False, "mixed16").nhood) == 16 and len({tuple(o) for o in TC.MIXED16}) == 16
    assert any(min(o) < 0 < max(o) for o in TC.MIXED) and any(min(o) > -1 and max(o) > 0 for o in TC.MIXED)
    for roi, name in ((False, "none"), (True, "none")):
        assert TC.aff_case(roi, name).unl is None
    c = TC.aff_case(True, "stack3d")
    assert c.labels.shape[:2] == (3, 5) and c.roi_offset[0] > 0 and not c.only_xy and c.steps == 2
    assert TC.aff_case(True, "stack3d_xy").only_xy


# ---- injected faults: what a wrong kernel would give is refused by the gate ---------------------------------------------
@pytest.mark.parametrize("nd,name,fault", [(3, "thin_origin", "count0_cell"), (3, "thin_offset", "count0_cell"),
                                           (2, "thin_origin", "count0_cell"), (2, "thin_offset", "count0_cell"),
                                           (3, "edge", "edge_replicate"), (2, "edge", "edge_replicate"), (2, "thin_origin", "edge_replicate"),
                                           (3, "df4", "second_label"), (3, "df8", "second_label"), (2, "df4", "second_label"),
                                           (2, "df8", "second_label")])
def test_lsd_gate_refuses_fault(nd, name, fault):
    c = TC.lsd_case(nd, name)
    ref, w = TC.lsd_reference(nd, name)
    bad = TC.lsd_direct_reference(nd, name, fault).astype(np.float32)
    err = np.abs(bad.astype(np.float64) - ref).max(axis=tuple(range(1, ref.ndim)))
    print(f"{nd}d-{name} with {fault}: largest error per channel", err)
    with pytest.raises(AssertionError):
        TC.gate_lsd(bad, w, ref, w, c.labels[c.roi])
    if fault == "count0_cell":     # the 3-D kernel before its count-0 rule followed the package: the offsets alone, by up to 0.5
        assert err[:nd].max() > 0.3 and err[nd:].max() < TC.LSD_ATOL


@pytest.mark.parametrize("nd", [3, 2])
def test_lsd_gate_refuses_labels_truncated_to_32_bits(nd):
    from lsd_direct_ref import lsd_direct, lsd_direct_sections
    c = TC.lsd_case(nd, "highbits")
    ref, w = TC.lsd_reference(nd, "highbits")
    bad = (lsd_direct if nd == 3 else lsd_direct_sections)(c.labels & 0xFFFFFFFF, c.roi_offset, c.roi_shape, c.sigma, c.voxel_size, c.df)
    with pytest.raises(AssertionError):
        TC.gate_lsd(bad.astype(np.float32), w, ref, w, c.labels[c.roi])


@pytest.mark.parametrize("roi,name,fault", [(False, "highbits", "trunc32"), (True, "highbits", "trunc32"),
                                            (False, "clip_low", "noclip"), (False, "clip_high", "noclip"), (True, "regimes", "noclip"),
                                            (True, "regimes", "section0"),
                                            (False, "product9", "neighbour_mask"), (False, "mixed", "neighbour_mask"), (True, "mixed", "neighbour_mask"),
                                            (True, "stack3d", "seam")])
def test_affinity_gate_refuses_fault(roi, name, fault):
    ref = TC.aff_reference(roi, name)
    TC.gate_affinity(ref["grown"], ref["affs"], ref["weights"], ref)
    bad = TC.aff_reference(roi, name, fault)
    with pytest.raises(AssertionError):
        TC.gate_affinity(bad["grown"], bad["affs"], bad["weights"], ref)
    if fault == "trunc32":         # the seam between objects equal in their low 32 bits: no erosion, affinity 1 across it
        assert (bad["grown"] != ref["grown"]).any() and (bad["affs"] > ref["affs"]).any()
    if fault in ("noclip", "section0", "neighbour_mask"):
        assert np.array_equal(bad["grown"], ref["grown"]) and np.array_equal(bad["affs"], ref["affs"])   # the weights alone
    if fault == "seam":
        assert (bad["grown"] != ref["grown"]).any()


def test_section_counters_fault_moves_every_other_section():
    """`regimes`: with section 0's counters every known section gets section 0's weights -- far beyond rtol 1e-6 in section 3"""
    ref, bad = TC.aff_reference(True, "regimes"), TC.aff_reference(True, "regimes", "section0")
    assert np.array_equal(bad["weights"][:, 0], ref["weights"][:, 0])
    m = ref["mask"][:, 3] > 0
    assert (np.abs(bad["weights"][:, 3][m] / ref["weights"][:, 3][m] - 1) > 1e-2).all()


@pytest.mark.parametrize("name", TC.SAT_NAMES)
def test_sat_fixtures_and_gate(name):
    m = TC.sat_case(name)
    ref = TC.sat_reference(m)
    TC.gate_sat(ref.copy(), ref)
    assert ref[:, -1, -1].tolist() == [int((sec != 0).sum()) for sec in m]
    if name == "values":
        assert m.shape == (3, 130, 300) and set(np.unique(m)) == {0, 1, 7, 255} and (m[1] == 1).all()
        assert m.shape[0] * (m.shape[1] + 1) > 256 and m.shape[0] * (m.shape[2] + 1) > 256
    if name != "ones":
        with pytest.raises(AssertionError):
            TC.gate_sat(TC.sat_reference(m, "sum"), ref)
