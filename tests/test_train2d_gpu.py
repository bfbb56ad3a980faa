"""`bs train` on the 2-D setups (2d_lsd, 2d_affs, 2d_mtlsd): the batched 2-D descriptor kernel and the affinities of a
section with context against their restatements, the training step on a stack of sections against the oracle's autograd of
the batched loss, and the driver end to end on a sparsely painted store."""
import glob
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _blob_sections(rng, s, h, w):
    """blob labels with background and a straight boundary, different in every section, touching every edge"""
    from scipy.ndimage import gaussian_filter
    out = np.zeros((s, h, w), np.int64)
    for i in range(s):
        blobs = gaussian_filter(rng.random((h, w)), 3 + i % 3)
        lab = (np.digitize(blobs, np.quantile(blobs, [0.2, 0.4, 0.6, 0.8])) + 1).astype(np.int64)
        lab[blobs < np.quantile(blobs, 0.1)] = 0                     # background
        lab[:, w * (i + 2) // (s + 3):] += 7 + 11 * i                 # more objects, a straight boundary
        out[i] = lab
    return out


@pytest.mark.parametrize("df,sigma,vs", [(2, (80.0, 80.0), (4.0, 4.0)), (1, (6.0, 6.0), (2.0, 2.0)), (2, (10.0, 12.0), (2.0, 3.0))])
def test_lsd2d_targets_vs_restatement(df, sigma, vs):
    """bsmi_train_lsd2d_targets on a batch of sections against tests/lsd2d_ref.py (the lsd package is absent: parity
    unpinned).  The kernel accumulates in f32 relative to the cell; the restatement filters in f64."""
    from bootstrapper_amd.train import lsd2d_targets
    from lsd2d_ref import lsd2d_targets as ref_lsd
    rng = np.random.default_rng(int(df * 100 + sigma[0]))
    ctx = [-(-int(-(-3.0 * s // v)) // df) * df for s, v in zip(sigma, vs)]
    roi = (40, 36)
    shape = (roi[0] + 2 * ctx[0], roi[1] + 2 * ctx[1])
    labels = _blob_sections(rng, 4, *shape)
    labels[1, :, : ctx[1] // 2] = 0                                   # a section whose labels stop inside the context
    unl = (rng.random(labels.shape) > 0.1).astype(np.uint8)
    lsds, w = lsd2d_targets(torch.from_numpy(labels).cuda(), ctx, roi, sigma, vs, df, torch.from_numpy(unl).cuda())
    ref, wref = ref_lsd(labels, ctx, roi, sigma, vs, df, unl)
    got = lsds.cpu().numpy()
    assert got.shape == (6, 4) + roi and np.array_equal(w.cpu().numpy(), wref)
    err = np.abs(got - ref).max(axis=(1, 2, 3))
    print("max abs error per channel", err)
    assert err.max() < 1e-4, err
    bg = labels[:, ctx[0]:ctx[0] + roi[0], ctx[1]:ctx[1] + roi[1]] == 0
    assert bg.any() and (got[:, bg] == 0).all()


def test_lsd2d_targets_rejects_bad_input():
    from bootstrapper_amd.train import lsd2d_targets
    lab = torch.ones((2, 40, 40), dtype=torch.int64, device="cuda")
    for args, msg in ((((4, 4), (30, 30), 10.0, (4, 4), 4), "multiples"), (((2, 2), (36, 36), 10.0, (4, 4), 3), "multiples"),
                      (((4, 4), (32, 32), 400.0, (1, 1), 1), "radius"), (((4, 4), (32, 32), -1.0, (4, 4), 2), "positive"),
                      (((4, 4), (32, 32), 10.0, (0, 4), 2), "positive")):
        with pytest.raises(RuntimeError, match=msg):
            lsd2d_targets(lab, *args)


@pytest.mark.parametrize("steps,with_mask", [(1, True), (0, False), (2, True)])
def test_affinity_targets_roi_vs_oracle(steps, with_mask):
    """Affinities of the output ROI of sections grown by the neighbourhood's context: oracle/train_ref on the grown section,
    cropped, with BalanceLabels restated on the crop of every section."""
    from bootstrapper_amd.train import affinity_targets_roi
    from oracle import train_ref as TR
    rng = np.random.default_rng(11 + steps)
    nhood2 = [[-1, 0], [0, -1], [-9, 0], [0, -9], [-27, 0], [0, -27]]
    nhood = [[0, *o] for o in nhood2]
    roi, lo = (40, 44), (27, 27)
    labels = _blob_sections(rng, 3, roi[0] + lo[0], roi[1] + lo[1])[:, None]
    unl = (labels > 0).astype(np.uint8)
    if with_mask:
        unl[0, 0, 30:40, 30:50] = 0
        unl[2, 0, :20, :] = 0
    lab_t = torch.from_numpy(labels.copy()).cuda()
    a, w = affinity_targets_roi(lab_t, torch.from_numpy(unl).cuda(), (0, lo[0], lo[1]), (1,) + roi, nhood, steps, only_xy=True)
    a, w = a.cpu().numpy(), w.cpu().numpy()
    assert a.shape == (6, 3, 1) + roi
    for s in range(3):
        grown = TR.grow_boundary(labels[s], unl[s], steps, True)
        affs, mask = TR.affinities_from_labels(grown, nhood)
        mask = mask * (unl[s] > 0)[None]
        crop = (slice(None), slice(None), slice(lo[0], None), slice(lo[1], None))
        affs, mask = affs[crop], mask[crop]
        assert np.array_equal(lab_t[s].cpu().numpy(), grown)
        assert np.array_equal(a[:, s], affs)
        assert np.allclose(w[:, s], TR.balance_labels(affs, mask), rtol=1e-6, atol=0)


def test_mask_sat_counts():
    from bootstrapper_amd.train import mask_sat
    rng = np.random.default_rng(3)
    m = (rng.random((3, 37, 53)) > 0.7).astype(np.uint8)
    sat = mask_sat(torch.from_numpy(m).cuda()).cpu().numpy()
    ref = np.zeros((3, 38, 54), np.int64)
    ref[:, 1:, 1:] = m.astype(np.int64).cumsum(1).cumsum(2)
    assert np.array_equal(sat, ref)


def test_training_step_on_section_stack_vs_oracle(golden_dir):
    """One step of the 2d_mtlsd_f4i2 family net on a stack of 4 sections: the loss and every gradient against the oracle's
    autograd of the reference's batched loss (a batch of 4 through the Conv2d net, one masked mean over it); the same
    step on one section equals the depth-1 result."""
    from bootstrapper_amd.unet import Model
    from bootstrapper_amd.training import Trainer
    from oracle import train_ref as T
    from oracle import unet_ref as R
    from test_oracle_unet import family_case
    nc, sd, _, x1, refs = family_case(golden_dir, "2d_mtlsd_f4i2")
    rng = np.random.default_rng(5)
    S = 4
    cin, H, W = x1.shape[1], x1.shape[3], x1.shape[4]
    x = np.concatenate([x1[0]] + [(rng.random((cin, 1, H, W), dtype=np.float32) * 2 - 1) for _ in range(S - 1)], axis=1)
    heads = [R.FAMILY_HEADS[k] for k in nc["outputs"]]
    lsd = {k: v.numpy() for k, v in R.lift_sd(sd).items()}
    m = Model(nc, precision="f32").load_state_dict(sd)
    tr = Trainer(m, (S, H, W), lr=1e-4, arithmetic="f32")
    shapes = [(r.shape[0], S) + r.shape[1:] for r in refs]
    targets = [rng.random(s, dtype=np.float32) for s in shapes]
    weights = [(rng.random(s, dtype=np.float32) * (rng.random(s) > 0.3)).astype(np.float32) for s in shapes]
    loss = tr.forward_backward(torch.from_numpy(x).cuda(), [torch.from_numpy(t).cuda() for t in targets], [torch.from_numpy(w).cuda() for w in weights])
    # the reference's batch: S sections through the unit-depth net, the loss over all of them at once
    ref_loss, ref_grads, _ = T.loss_and_grads(R.lift_cfg(nc), lsd, x, [t[None] for t in targets], [w[None] for w in weights], heads)
    assert abs(loss - ref_loss) < 1e-5 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    worst = 0.0
    for k, g in ref_grads.items():
        err = np.abs(tr.read(k, "grad") - g.ravel()).max() / max(1e-6, np.abs(g).max())
        worst = max(worst, err)
        assert err < 1e-3, (k, err)
    print(f"stack of {S}: loss {loss:.6f}, largest relative gradient error {worst:.2e}")
    tr.close()
    # one section through the 2-D settings path: the depth-1 step of the existing family test
    m = Model(nc, precision="f32").load_state_dict(sd)
    tr = Trainer(m, (1, H, W), lr=1e-4, arithmetic="f32")
    loss1 = tr.forward_backward(torch.from_numpy(x[:, :1].copy()).cuda(), [torch.from_numpy(t[:, :1].copy()).cuda() for t in targets],
                                [torch.from_numpy(w[:, :1].copy()).cuda() for w in weights])
    ref1, g1, _ = T.loss_and_grads(R.lift_cfg(nc), lsd, x[:, :1].copy(), [t[None, :, :1] for t in targets], [w[None, :, :1] for w in weights], heads)
    assert abs(loss1 - ref1) < 1e-5 * max(1.0, abs(ref1)), (loss1, ref1)
    for k, g in g1.items():
        assert np.abs(tr.read(k, "grad") - g.ravel()).max() / max(1e-6, np.abs(g).max()) < 1e-3, k
    tr.close()


def _store(tmp_path, rng):
    """raw (90, 200, 200) at world offset 0; labels + mask a bounding-box crop (60, 150, 160) at a non-zero offset, painted
    on one section in 60 (and only inside it), voxel size (40, 4, 4)"""
    from bootstrapper_amd.zarr_io import prepare_ds
    store = str(tmp_path / "cremi.zarr")
    vs = (40, 4, 4)
    raw = rng.integers(0, 256, size=(90, 200, 200), dtype=np.uint8)
    ds = prepare_ds(f"{store}/raw", raw.shape, offset=(0, 0, 0), voxel_size=vs, chunk_shape=(8, 64, 64), dtype=np.uint8)
    ds[:] = raw
    loff = (10, 20, 24)   # voxels
    labels = np.zeros((60, 150, 160), np.uint64)
    mask = np.zeros(labels.shape, np.uint8)
    painted = [37]
    for z in painted:
        lab = _blob_sections(rng, 1, 150, 160)[0]
        labels[z] = lab.astype(np.uint64)
        mask[z] = 1
    for name, arr in (("labels", labels), ("labels_mask", mask)):
        ds = prepare_ds(f"{store}/{name}", arr.shape, offset=[o * v for o, v in zip(loff, vs)], voxel_size=vs, chunk_shape=(8, 64, 64),
                        dtype=arr.dtype)
        ds[:] = arr
    return store, raw, labels, loff, painted


def _setup(tmp_path, name, outputs):
    setup = tmp_path / name
    setup.mkdir()
    nc = {"in_channels": 1, "adj_slices": 3, "num_fmaps": 4, "fmap_inc_factor": 2, "downsample_factors": [[2, 2], [2, 2], [2, 2]],
          "kernel_size_down": [[[3, 3], [3, 3]]] * 4, "kernel_size_up": [[[3, 3], [3, 3]]] * 3,
          "input_shape": [108, 108], "output_shape": [16, 16], "inputs": {"raw": {"dims": 1}}, "outputs": outputs}
    (setup / "net_config.json").write_text(json.dumps(nc))
    return setup, nc


OUTS = {"2d_mtlsd": {"2d_lsds": {"dims": 6, "sigma": 80, "downsample": 2},
                     "2d_affs": {"dims": 6, "neighborhood": [[-1, 0], [0, -1], [-9, 0], [0, -9], [-27, 0], [0, -27]], "grow_boundary": 1}},
        "2d_lsd": {"2d_lsds": {"dims": 6, "sigma": 80, "downsample": 2}}}


@pytest.mark.parametrize("name", ["2d_mtlsd", "2d_lsd"])
def test_bs_train_2d_end_to_end(tmp_path, name):
    from bootstrapper_amd.train import make_sample_source, run_training, latest_checkpoint, setup_train
    from bootstrapper_amd.unet import Model
    from bootstrapper_amd.zarr_io import open_ds
    rng = np.random.default_rng(8)
    store, raw, labels, loff, painted = _store(tmp_path, rng)
    setup, nc = _setup(tmp_path, f"setup_{name}", OUTS[name])
    cfg = tmp_path / "train.toml"
    cfg.write_text(f'setup_dir = "{setup}"\nvoxel_size = [40, 4, 4]\nmax_iterations = 3\nsave_checkpoints_every = 3\nsave_snapshots_every = 1000\n'
                   f'[[samples]]\nraw = "{store}/raw"\nlabels = "{store}/labels"\nmask = "{store}/labels_mask"\n')
    config = setup_train(str(cfg))
    src, src2 = make_sample_source(config, nc, 0, 0), make_sample_source(config, nc, 0, 0)
    a, b = next(src), next(src2)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)          # same seed, same batches
    assert tuple(a["raw"].shape) == (3, 10, 108, 108)
    assert tuple(a["gt_lsds"].shape) == (6, 10, 16, 16) and tuple(a["lsds_weights"].shape) == (6, 10, 16, 16)
    assert float(a["gt_lsds"].max()) <= 1.0 and float(a["lsds_weights"].sum()) > 0
    if name == "2d_mtlsd":
        assert tuple(a["gt_affs"].shape) == (6, 10, 16, 16) and tuple(a["affs_weights"].shape) == (6, 10, 16, 16)
    # every draw is a painted section; its raw is the raw dataset at that section's world position (labels offset + draw)
    rs = np.random.default_rng(42)
    rawp = np.pad(raw, ((0, 0), (64, 64), (64, 64)))
    for s in range(10):
        while True:
            rs.integers(1)
            z, y, x = (int(rs.integers(0, n - o + 1)) for n, o in zip(labels.shape, (1, 16, 16)))
            if z in painted:
                break
        Y, X = loff[1] + y + 64, loff[2] + x + 64
        want = rawp[loff[0] + z - 1:loff[0] + z + 2, Y - 46:Y + 62, X - 46:X + 62]
        got = np.rint((a["raw"][:, s].cpu().numpy() + 1) / 2 * 255).astype(np.uint8)
        assert np.array_equal(got, want), s
        lw = a["lsds_weights"][0, s].cpu().numpy()
        assert np.array_equal(lw > 0, labels[z, y:y + 16, x:x + 16] > 0)
    # run the driver: 3 iterations, snapshots at step 1, a checkpoint the predict-side Model loads
    cfg.write_text(cfg.read_text().replace("save_snapshots_every = 1000", "save_snapshots_every = 2"))
    logs = []
    assert run_training(str(cfg), log=logs.append) == 3
    ckpt, step = latest_checkpoint(str(setup))
    assert step == 3
    snap = str(setup / "snapshots" / "batch_1_rank_0.zarr")
    assert os.path.isdir(snap)
    pred = open_ds(snap + "/pred_lsds")
    assert pred.shape == (10, 6, 1, 16, 16)
    assert open_ds(snap + "/raw").shape == (10, 3, 108, 108)
    ck = torch.load(ckpt, map_location="cpu", weights_only=True)["state_dict"]
    assert ck["model.unet.l_conv.0.conv_pass.0.weight"].dim() == 4                      # Conv2d shapes
    m = Model(nc, precision="f32").load_checkpoint(ckpt)
    y = m(torch.zeros(1, 3, 108, 108, device="cuda"))
    y = y[0] if isinstance(y, tuple) else y
    assert tuple(y.shape)[-2:] == (16, 16) and bool(torch.isfinite(y).all())
    assert glob.glob(str(setup / "log" / "version_0" / "events.out.tfevents.*"))
