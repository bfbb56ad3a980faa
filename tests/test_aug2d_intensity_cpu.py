"""The intensity chain of the 2-D setups without a GPU: the train config key inside `[augment2d]` and its refusals, the
adj_slices-dependent default of prob_missing, the draw order inside SectionSource._next_augmented replayed by hand with the
device calls stubbed, the packed tables, and the comparisons of tests/test_aug2d_intensity_gpu.py run on a float32 emulation
of the batched launches -- which they must pass, and must not pass with any of the injected indexing faults."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug2d_intensity_ref as R2  # noqa: E402
from bootstrapper_amd import augment as G  # noqa: E402
from bootstrapper_amd import augment2d as A  # noqa: E402


# ---- the key ----

def test_the_key_and_its_defaults():
    assert A.Aug2DParams().intensity is None and A.Aug2DParams.from_config(True).intensity is None
    assert A.Aug2DParams.from_config({"intensity": False}).intensity is None
    p = A.Aug2DParams.from_config({"intensity": True})
    assert p.intensity.prob_missing is None                                   # open until adj_slices is known
    assert p.intensity_for(3) == dataclasses.replace(G.IntensityParams(), prob_missing=0.05)
    assert p.intensity_for(1) == dataclasses.replace(G.IntensityParams(), prob_missing=0.0)
    assert p.intensity_for(3).prob_low_contrast == 0.1
    assert G.IntensityParams().prob_missing == 0.1                            # the 3-D call site's default stays
    assert A.Aug2DParams().intensity_for(3) is None
    q = A.Aug2DParams.from_config({"deform_p": 0.25, "intensity": {"prob_missing": 0.2, "noise_p": 0.0, "blur": [0.5, 1.0]}})
    assert q.deform_p == 0.25 and q.intensity_for(1).prob_missing == 0.2 and q.intensity_for(3).prob_missing == 0.2
    assert q.intensity.noise_p == 0.0 and q.intensity.blur == (0.5, 1.0)
    # a table without prob_missing: the other keys are taken, the default stays open
    r = A.Aug2DParams.from_config({"intensity": {"prob_low_contrast": 0.5}})
    assert r.intensity_for(1).prob_missing == 0.0 and r.intensity_for(2).prob_missing == 0.05 and r.intensity.prob_low_contrast == 0.5


@pytest.mark.parametrize("table,match", [
    ({"noise_p": 2}, r"augment2d\.intensity\.noise_p .*a probability"),
    ({"nois_p": 0.5}, r"unknown augment2d\.intensity key\(s\) nois_p"),
    ({"blur": [0.5, 2.0]}, r"augment2d\.intensity\.blur .*radius"),
    ({"scale": [1.1, 0.9]}, r"augment2d\.intensity\.scale .*low <= high"),
    ({"prob_missing": 0.6, "prob_low_contrast": 0.6}, r"augment2d\.intensity: prob_missing \+ prob_low_contrast exceeds 1"),
    ({"prob_low_contrast": 0.99}, r"augment2d\.intensity: prob_missing \+ prob_low_contrast exceeds 1"),   # with the default 0.05
    (3, r"augment2d\.intensity must be true, false or a table"),
])
def test_refused_tables_name_the_key(table, match):
    with pytest.raises(ValueError, match=match):
        A.Aug2DParams.from_config({"intensity": table})
    # the 3-D key's own texts are unchanged
    if isinstance(table, dict) and "prob_low_contrast" not in table:
        with pytest.raises(ValueError, match=match.replace("augment2d", "augment")):
            G.AugParams.from_config({"intensity": table})


def test_the_other_refusals_stay():
    from bootstrapper_amd.train import make_sample_source
    two_d = {"downsample_factors": [[2, 2]], "input_shape": [48, 48], "output_shape": [32, 32], "outputs": {"2d_lsds": {"dims": 6, "sigma": 40}}}
    three_d = {"downsample_factors": [[1, 2, 2]], "input_shape": [8, 48, 48], "output_shape": [4, 32, 32], "outputs": {"3d_affs": {"dims": 3}}}
    with pytest.raises(NotImplementedError, match="2-D setups"):
        make_sample_source({"augment": {"intensity": True}, "samples": []}, two_d)
    with pytest.raises(NotImplementedError, match="augment2d: not built"):
        make_sample_source({"augment2d": {"intensity": True}, "samples": []}, three_d)
    assert "Clahe" in A.NOT_BUILT and "DefectAugment" in A.NOT_BUILT and "NoiseAugment" not in A.NOT_BUILT


# ---- the packed tables ----

def test_packed_tables():
    x, plans = R2.build_case("S3_K3_24x24")
    S, K = 3, 3
    t = A.PackedIntensity2D(plans)
    assert (t.S, t.K, t.section) == (S, K, (24, 24)) and t.planes.shape == (4, K * S) and t.planes.dtype == np.int32
    assert t.touched == [p.applied for p in plans] == [True, False, True]
    assert [d.nodes for d in t.idraws] == [127, 0, A.SMOOTH | A.TOUCHED] and t.nodes == 127 and t.low_contrast
    fl = t.planes.view(np.float32)
    for k in range(K):
        for s, plan in enumerate(plans):
            p = k * S + s                                                      # the plane of section k of draw s in [K][S][H][W]
            assert fl[0, p] == (plan.scale[k] if plan.scale is not None else 1.0) and fl[1, p] == (plan.shift[k] if plan.shift is not None else 0.0)
            assert fl[2, p] == (plan.gamma[k] if plan.gamma is not None else 1.0) and t.planes[3, p] == (plan.defect[k] if plan.defect is not None else 0)
    d0, d2 = t.idraws[0], t.idraws[2]
    assert (d0.radius, d0.taps_offset, d2.radius, d2.taps_offset) == (6, 0, 2, 13) and t.taps.size == 13 + 5 and t.taps.dtype == np.float32
    assert np.array_equal(t.taps[:13], plans[0].weights) and np.array_equal(t.taps[13:], plans[2].weights)
    assert d0.seed == plans[0].seed and d0.impulse_threshold == 2 ** 31 and d0.noise_sigma == np.float32(0.1) and d0.contrast_scale == np.float32(0.1)
    assert C_sizeof(d0) == 48
    with pytest.raises(ValueError, match="share one stack shape"):
        A.PackedIntensity2D([plans[0], G.IntensityPlan((3, 24, 25))])
    none = A.PackedIntensity2D([G.IntensityPlan((3, 8, 8))] * 2)
    assert none.nodes == 0 and none.taps is None and none.touched == [False, False]
    assert A.apply_intensity2d("never looked at", none) == "never looked at"     # no touched draw: no launch, no tensor needed


def C_sizeof(struct):
    import ctypes
    return ctypes.sizeof(struct)


# ---- the emulation passes the GPU test's comparisons, and fails them with every injected fault ----

@pytest.mark.parametrize("case", sorted(R2.CASES))
def test_emulation_passes_the_comparisons(case):
    x, plans = R2.build_case(case)
    R2.compare(R2.Emulated(A.PackedIntensity2D(plans)), x, plans, R2.EmulatedBlock(), show=lambda line: None)


@pytest.mark.parametrize("fault", R2.FAULTS)
def test_every_injected_fault_fails_the_comparisons(fault):
    x, plans = R2.build_case("S3_K3_24x24")
    with pytest.raises(AssertionError):
        R2.compare(R2.Emulated(A.PackedIntensity2D(plans), fault), x, plans, R2.EmulatedBlock(), show=lambda line: None)


# ---- the draws of SectionSource._next_augmented, with the device calls stubbed ----

def _stub_source(monkeypatch, intensity, reject):
    """A SectionSource built without a store or a device: the location draws take two numbers from the stream, the device calls
    return host tensors, and the round's counts fail the slots in `reject` (first round only).  -> (source, events)"""
    import torch
    from bootstrapper_amd import train as T
    events = []
    src = T.SectionSource.__new__(T.SectionSource)
    src.augment = A.Aug2DParams(simple=True, deform_p=0.0, shift_p=0.0, intensity=intensity)
    src.intensity = src.augment.intensity_for(3)
    src.batch_size, src.adj, src.inp, src.out, src.ctx = 4, 3, (16, 16), (8, 8), [4, 4]
    src.lo, src.hi, src.vs, src.dev = [0, 0], [0, 0], (40, 4, 4), torch.device("cpu")
    src.frame = A.frame_of(src.inp, src.out, src.lo, src.hi)
    src.rng = np.random.default_rng(3)
    ds = type("DS", (), {"voxel_size": (40, 4, 4), "offset": (0, 0, 0), "dtype": np.uint64})()
    src.samples = [(ds, ds, None)]
    rounds = [0]

    def draw():
        events.append("location")
        return 0, int(src.rng.integers(100)), int(src.rng.integers(100)), 0
    monkeypatch.setattr(src, "_draw", draw, raising=False)
    monkeypatch.setattr(src, "_known", lambda i, start, shape: np.ones(shape, dtype=np.uint8), raising=False)
    monkeypatch.setattr(src, "_targets", lambda lab, unl: {}, raising=False)
    monkeypatch.setattr(T, "_read_world", lambda ds, world, shape, dtype: np.zeros(shape, dtype=dtype))
    real_plan, real_iplan = A.draw_plan2d, G.draw_intensity_plan
    monkeypatch.setattr(A, "draw_plan2d", lambda *a, **k: (events.append("plan"), real_plan(*a, **k))[1])
    monkeypatch.setattr(G, "draw_intensity_plan", lambda rng, params, shape: (events.append(("intensity plan", tuple(shape))), real_iplan(rng, params, shape))[1])
    monkeypatch.setattr(A, "coords2d", lambda packed, dev: torch.zeros(1))

    def nearest(fill):
        def fn(packed, coords, crops, window):
            n = packed.S
            out = torch.full((n,) + tuple(window[1]), fill, dtype=torch.int64 if fill == 7 else torch.uint8)
            if fill == 1:
                events.append("mask launch")
                if rounds[0] == 0:
                    for j in reject:
                        out[j] = 0
                rounds[0] += 1
            return out
        return fn
    monkeypatch.setattr(A, "sample_labels2d", nearest(7))
    monkeypatch.setattr(A, "sample_mask2d", nearest(1))

    def raw(kind):
        def fn(packed, coords, crops, *rest):
            ipacked = rest[0] if kind == "unit" else None
            events.append((kind + " raw launch", None if ipacked is None else tuple(ipacked.touched)))
            return torch.zeros((packed.K, packed.S) + src.inp)
        return fn
    monkeypatch.setattr(A, "sample_raw2d", raw("final"))
    monkeypatch.setattr(A, "sample_unit2d", raw("unit"))
    monkeypatch.setattr(A, "apply_intensity2d", lambda raw_t, packed: (events.append(("chain", tuple(packed.touched), packed.S)), raw_t)[1])
    return src, events


def test_no_intensity_draw_without_the_key(monkeypatch):
    """without `intensity` the round is today's: the raw launch before the read-back, not one draw more"""
    src, events = _stub_source(monkeypatch, None, reject=[1])
    twin = np.random.default_rng(3)
    src._next_augmented()
    assert not [e for e in events if isinstance(e, tuple) and e[0] in ("intensity plan", "unit raw launch", "chain")]
    assert [e for e in events if e not in ("location", "plan")] == ["mask launch", ("final raw launch", None)] * 2
    for _ in range(4 + 1):                                                     # four slots, then slot 1 again: location (2 numbers), plan (4 coins)
        twin.integers(100), twin.integers(100)
        [twin.random() for _ in range(4)]
    assert src.rng.bit_generator.state == twin.bit_generator.state


def test_intensity_draws_follow_the_read_back_for_accepted_slots_in_slot_order(monkeypatch):
    params = dataclasses.replace(G.IntensityParams(), prob_missing=None)
    src, events = _stub_source(monkeypatch, params, reject=[1, 2])
    twin = np.random.default_rng(3)
    src._next_augmented()
    # round 1: four (location, plan), the mask launch (whose counts are read back), then the plans of slots 0 and 3 only, then raw
    shape = ("intensity plan", (3, 16, 16))
    assert events[:8] == ["location", "plan"] * 4
    assert events[8:11] == ["mask launch", shape, shape] and events[11][0] == "unit raw launch" and events[11][1][1:3] == (False, False)
    # round 2: slots 1 and 2 again
    assert events[12:16] == ["location", "plan"] * 2 and events[16:19] == ["mask launch", shape, shape] and events[19][0] == "unit raw launch"
    assert events[20][0] == "chain" and events[20][2] == 4 and len(events) == 21
    # the stream, by hand: a rejected slot takes no intensity draw
    resolved = src.intensity
    assert resolved.prob_missing == 0.05

    def geometry(n):
        for _ in range(n):
            twin.integers(100), twin.integers(100)
            [twin.random() for _ in range(4)]
    geometry(4)
    first = [_draw(twin, resolved) for _ in range(2)]
    geometry(2)
    second = [_draw(twin, resolved) for _ in range(2)]
    assert src.rng.bit_generator.state == twin.bit_generator.state
    # the chain's table holds the plan every slot was accepted with: slots 0, 3 from round 1, slots 1, 2 from round 2
    assert events[20][1] == tuple(p.applied for p in (first[0], second[0], second[1], first[1]))
    assert events[11][1] == (first[0].applied, False, False, first[1].applied) and events[19][1] == tuple(p.applied for p in second)


def _draw(rng, params):
    """augment.draw_intensity_plan's draws, restated from its docstring: only the stream matters here, and `applied`"""
    d = 3
    plan = G.IntensityPlan((3, 16, 16))
    if rng.random() < params.noise_p:
        plan.noise_sigma = 0.1
    if rng.random() < params.intensity_p:
        plan.scale, plan.shift = rng.uniform(*params.scale, d), rng.uniform(*params.shift, d)
    if rng.random() < params.gamma_p:
        plan.gamma = rng.uniform(*G.gamma_interval(params.gamma), d)
    if rng.random() < params.impulse_p:
        plan.impulse_threshold = 1
    if rng.random() < params.smooth_p:
        plan.weights = rng.uniform(*params.blur)
    r = rng.random(d)
    rng.random(d)
    if (r < params.prob_missing + params.prob_low_contrast).any():
        plan.defect = r
    if plan.noise_sigma is not None or plan.impulse_threshold is not None:
        rng.integers(0, 2 ** 64, dtype=np.uint64)
    return plan
