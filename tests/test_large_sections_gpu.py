"""Non-blockwise watershed on full-size sections: slices of 2^20 voxels and more (CREMI's 1250 x 1250) take the wide flood
(csrc/seg_ws.hip: ws_flood_wide_kernel), 3-D volumes of 2^23 voxels and more the wide host flood (csrc/flood_host.cpp); both
bit-exact against the C oracle.  Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _blobby(rng, shape, sigma):
    from scipy.ndimage import gaussian_filter
    a = gaussian_filter(rng.random((3,) + shape, dtype=np.float32), sigma=(0,) + sigma)
    a = (a - a.min()) / (a.max() - a.min())
    return (a * 255).astype(np.uint8)


def _case(kind, shape):
    rng = np.random.default_rng(sum(shape) + len(kind))
    if kind == "blobby":
        return _blobby(rng, shape, (0, 6, 6))
    if kind == "noise":      # a seed every few voxels: a deep heap
        return rng.integers(0, 256, (3,) + shape, dtype=np.uint8)
    a = np.zeros((3,) + shape, np.uint8)
    if kind == "half":       # one straight edge: distance plateaus along it, seeds tied in d2
        a[:, :, :, : shape[2] // 2] = 255
    elif kind == "full":     # no background: scipy's distances from (-1, 0), up to H^2 + W^2
        a[:] = 255
    return a                 # "empty": all background, no fragment


def _check_fragments(affs, msd, return_seeds=False):
    from bootstrapper_amd.post.ws import watershed_from_affinities
    from oracle import seg_ref as S
    got = watershed_from_affinities(torch.from_numpy(affs).cuda(), fragments_in_xy=True, min_seed_distance=msd,
                                    return_seeds=return_seeds)
    ref = S.ws_fragments_u8(affs, True, msd, return_seeds=return_seeds)
    assert got[1] == ref[1]
    assert np.array_equal(got[0].cpu().numpy().astype(np.uint64), ref[0])
    if return_seeds:
        assert np.array_equal(got[2].cpu().numpy().astype(np.uint64), ref[2])
    return ref


@pytest.mark.parametrize("kind,shape,msd", [
    ("blobby", (4, 1250, 1250), 10),     # CREMI sections
    ("blobby", (2, 1024, 1024), 10),     # exactly 2^20 voxels: the first size the packed flood entry cannot take
    ("blobby", (1, 1100, 1900), 10),     # not square
    ("blobby", (1, 260, 4096), 10),      # W at the max_shape bound: the flood's row index
    ("noise", (1, 1024, 1200), 2),
    ("half", (1, 1250, 1250), 10),
    ("full", (1, 1250, 1250), 10),
    ("empty", (1, 1024, 1024), 10),
])
def test_wide_fragments_bit_exact_vs_oracle(kind, shape, msd):
    _check_fragments(_case(kind, shape), msd)


def test_wide_fragments_with_seeds_bit_exact_vs_oracle():
    _check_fragments(_case("blobby", (2, 1030, 1100)), 8, return_seeds=True)


def test_wide_fragments_heap_past_the_second_spill_window():
    """White noise on 2048^2 at msd 2: more than 2^18 - 1 seeds are queued up front, so the heap reaches depth 18 and
    sift-downs cross into the second five-level window of spilled nodes (rooted at depth 17, owner lanes wrapping)."""
    affs = _case("noise", (1, 2048, 2048))
    _, mx = _check_fragments(affs, 2)
    assert mx > (1 << 18)


def test_wide_slices_are_laid_out_within_4096_per_axis():
    """A call may lay a handle's slice area out differently (check_seg_shape bounds H * W, not each axis).  A slice of 2^20
    voxels or more with H, W <= 4096 floods bit-exactly; with a row longer than 4096 -- beyond the wide flood's row index
    and distance keys -- the call is refused, as it was before the wide flood existed."""
    from bootstrapper_amd.post.engine import SegEngine
    from oracle import seg_ref as S
    eng = SegEngine((1, 1024, 1024), 0)
    affs = _blobby(np.random.default_rng(7), (1, 256, 4096), (0, 4, 4))
    frags, mx = eng.ws_fragments(torch.from_numpy(affs).cuda(), True, 10)
    ref, ref_max = S.ws_fragments_u8(affs, True, 10)
    assert int(mx.item()) == ref_max and np.array_equal(frags.cpu().numpy().astype(np.uint64), ref)
    for shape in ((1, 128, 8192), (1, 1, 1 << 20), (1, 8192, 128)):
        with pytest.raises(Exception, match="4096"):
            eng.ws_fragments(torch.zeros((3,) + shape, dtype=torch.uint8, device="cuda"), True, 10)
    torch.cuda.synchronize()
    # the handle still works after the refusals
    frags, mx = eng.ws_fragments(torch.from_numpy(affs).cuda(), True, 10)
    assert int(mx.item()) == ref_max and np.array_equal(frags.cpu().numpy().astype(np.uint64), ref)


def test_wide_handle_runs_small_shapes_as_before():
    """A handle sized for full sections still floods small slices (the packed-entry kernels) bit-exactly."""
    from bootstrapper_amd.post.engine import SegEngine
    from oracle import seg_ref as S
    eng = SegEngine((2, 1250, 1250), 0)
    for shape in ((2, 160, 160), (1, 700, 900)):
        affs = _blobby(np.random.default_rng(shape[1]), shape, (0, 3, 3))
        frags, mx = eng.ws_fragments(torch.from_numpy(affs).cuda(), True, 6)
        ref, ref_max = S.ws_fragments_u8(affs, True, 6)
        assert int(mx.item()) == ref_max and np.array_equal(frags.cpu().numpy().astype(np.uint64), ref)


def test_wide_agglomeration_bit_exact_vs_oracle():
    from bootstrapper_amd.post.engine import SegEngine
    from oracle import seg_ref as S
    affs = _case("blobby", (4, 1250, 1250))
    thr = [0.2, 0.35, 0.5]
    eng = SegEngine(affs.shape[1:], 0)
    a = torch.from_numpy(affs).cuda()
    frags, mx = eng.ws_fragments(a, True, 10)
    ref_frags, ref_max = S.ws_fragments_u8(affs, True, 10)
    assert int(mx.item()) == ref_max and np.array_equal(frags.cpu().numpy().astype(np.uint64), ref_frags)
    segs = eng.agglomerate_mean(a, frags, thr)
    eng.status()
    for s, r in zip(segs, S.agglomerate_mean_u8(affs, ref_frags, thr)):
        assert np.array_equal(s.cpu().numpy().astype(np.uint64), r)
    segs = eng.agglomerate_hist(a, frags, thr, 50)
    eng.status()
    for s, r in zip(segs, S.agglomerate_hist_u8(affs, ref_frags, thr, 50)):
        assert np.array_equal(s.cpu().numpy().astype(np.uint64), r)


def test_simple_watershed_on_full_sections(tmp_path):
    """`bs segment --ws` without blockwise on a (3, 4, 1250, 1250) store: the whole ROI, a sub-ROI with a mask, and the same
    store written as float32 u8 / 255 -> fragments and three segmentations equal to the oracle, bs_params written."""
    from bootstrapper_amd.post.watershed import simple_watershed
    from bootstrapper_amd.zarr_io import open_ds, prepare_ds
    from oracle import seg_ref as S
    affs = _case("blobby", (4, 1250, 1250))
    thr = [0.2, 0.35, 0.5]
    store = str(tmp_path / "vol.zarr")
    kw = dict(offset=(0, 0, 0), voxel_size=(40, 4, 4), units=["nm"] * 3)
    ds = prepare_ds(store + "/affs", affs.shape, axis_names=["c^", "z", "y", "x"], chunk_shape=(3, 2, 512, 512), dtype=np.uint8, **kw)
    ds[:] = affs
    dsf = prepare_ds(store + "/affs_f32", affs.shape, axis_names=["c^", "z", "y", "x"], chunk_shape=(3, 2, 512, 512),
                     dtype=np.float32, **kw)
    dsf[:] = affs.astype(np.float32) / np.float32(255)
    mask = np.ones(affs.shape[1:], np.uint8)
    mask[:, 200:500, 300:900] = 0
    dm = prepare_ds(store + "/mask", mask.shape, axis_names=["z", "y", "x"], chunk_shape=(2, 512, 512), dtype=np.uint8, **kw)
    dm[:] = mask

    def run(name, extra):
        cfg = {"affs_dataset": store + "/" + name, "fragments_dataset": f"{store}/{name}_out/fragments",
               "seg_dataset_prefix": f"{store}/{name}_out/segmentations", "thresholds": thr, "min_seed_distance": 10, **extra}
        written = simple_watershed(cfg)
        assert len(written) == 4
        for w in written:
            assert open_ds(w).attrs["bs_params"]["method"] == "ws" and open_ds(w).attrs["bs_params"]["blockwise"] is False
        return [open_ds(w)[:] for w in written], [open_ds(w).offset for w in written]

    def check(outs, a):
        ref_frags, _ = S.ws_fragments_u8(a, True, 10)
        assert np.array_equal(outs[0], ref_frags)
        for o, r in zip(outs[1:], S.agglomerate_mean_u8(a, ref_frags, thr)):
            assert np.array_equal(o, r)

    whole, offs = run("affs", {})
    assert all(tuple(o) == (0, 0, 0) for o in offs)
    check(whole, affs)
    sub, offs = run("affs", {"roi_offset": [40, 400, 0], "roi_shape": [120, 4400, 5000], "mask_dataset": store + "/mask"})
    assert all(tuple(o) == (40, 400, 0) for o in offs)
    check(sub, affs[:, 1:, 100:1200, :] * mask[None, 1:, 100:1200, :])
    as_float, _ = run("affs_f32", {})
    assert all(np.array_equal(a, b) for a, b in zip(as_float, whole))
    # continuous floats are refused: the device agglomeration scores uint8 affinities
    dsc = prepare_ds(store + "/affs_cont", (3, 1, 64, 64), axis_names=["c^", "z", "y", "x"], chunk_shape=(3, 1, 64, 64),
                     dtype=np.float32, **kw)
    dsc[:] = np.full((3, 1, 64, 64), 0.3, np.float32)
    with pytest.raises(NotImplementedError, match="uint8"):
        run("affs_cont", {})


def test_3d_mode_above_the_packed_entry():
    """fragments_in_xy = false on 210^3 (9.3 M voxels > 2^23): the host flood's wide entry, bit-exact; the device flood
    (host_flood = False) keeps its limit and refuses the shape."""
    from bootstrapper_amd.post.engine import SegEngine
    from bootstrapper_amd.post.ws import watershed_from_affinities
    from oracle import seg_ref as S
    affs = _blobby(np.random.default_rng(210), (210, 210, 210), (3, 3, 3))
    frags, mx = watershed_from_affinities(torch.from_numpy(affs).cuda(), fragments_in_xy=False, min_seed_distance=10)
    ref, ref_max = S.ws_fragments_u8(affs, False, 10)
    assert mx == ref_max and ref_max > 100
    assert np.array_equal(frags.cpu().numpy().astype(np.uint64), ref)
    eng = SegEngine(affs.shape[1:], 0, host_flood=False)
    with pytest.raises(Exception, match="2\\^23"):
        eng.ws_fragments(torch.from_numpy(affs).cuda(), False, 10)


def test_wide_flood_between_guard_zones():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BSMI_GUARD_MB="4")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "large_sections_guard_worker.py")], env=env,
                       capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0 and "guards intact" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
