"""`bs train` on the device: config checks, a minimal sample source and the training loop.

Reference being mirrored (paths relative to /root/reference/bootstrapper):
  train.py:13-120                 setup_train: sample path checks (same error texts), setup_dir / iteration settings
  models/3d_affs/train.py:160-199 train(setup_dir, voxel_size, max_iterations, samples, save_checkpoints_every, ...)
  training.py:96-137              fit(): seed 42, checkpoints `model_checkpoint_<step>`, resume from the latest one

What is NOT restated: DefectAugment's deformation and artifacts, and the snapshot callback -- third-party pipeline code
outside the hot path.  `SampleSource` does the deterministic part: random location with the >= 5 % labelled-voxel rejection, Normalize +
IntensityScaleShift(2, -1), then GrowBoundary, AddAffinities on the configured neighbourhood and BalanceLabels in one
device call (`affinity_targets`).  With the train config key `augment` it also applies the geometric chain of
models/3d_affs/train.py:95-104 (SimpleAugment -> DeformAugment -> ShiftAugment) on the device, as one coordinate map
(augment.py, csrc/augment.hip; specified rules), and with `intensity` inside that table the
intensity nodes of models/3d_affs/train.py:105-120 on raw (noise / intensity / gamma / impulse / smooth / defect: a launch
per node, csrc/augment_intensity.hip; specified rules, section 7k); without the key the batches are un-augmented crops,
as before.  `SectionSource`
does the same for the 2-D setups (models/2d_mtlsd/train.py:29-164): ten sections per batch, Add2DLSDs and the affinities
of each section in one launch each (csrc/train2d.hip); with the train config key `augment2d` the geometric chain of
models/2d_mtlsd/train.py:112-122 runs on the whole batch first, one coordinate launch and one resampling launch per array
for the ten draws (augment2d.py, csrc/augment2d.hip; specified rules, section 7l), and with `intensity` inside that table the
intensity nodes of raw after it, one launch per node for the ten draws (csrc/augment2d_intensity.hip; section 7m).
`SyntheticSource` feeds the second-stage setups (models/3d_affs_from_*/train.py) from labels made on the device (synth_labels.py, csrc/synth.hip), with
`synthetic_labels = true` in the train config; with `input_augment` beside it every input array runs through the reference's degradation of
the inputs (noise, intensity per channel and per section, smoothing per section, low contrast: augment_inputs.py, csrc/augment_inputs.hip;
specified rules, section 7n), and with `label_augment` the labels themselves run through SimpleAugment -> DeformAugment -> ShiftAugment
directly after they are created, zeros entering from outside the block (augment_labels.py, the launches of csrc/augment.hip; section 7o).
The arithmetic of the step itself is libbsmi (csrc/train*.hip; the targets: csrc/train_targets.hip).
"""
import ctypes as C
import glob
import json
import os
import random
import re

import numpy as np
import torch

try:
    import tomllib as _toml
except ImportError:  # python < 3.11
    import tomli as _toml

from . import _lib
from .zarr_io import open_ds


def setup_train(config_file):
    """train.py:13-120: load the TOML, check the sample datasets, return the config."""
    with open(config_file, "rb") as f:
        config = _toml.load(f)
    samples = config.get("samples", [])
    if "samples" in config and not samples:
        raise ValueError(f"No training samples provided in {config_file}")
    for sample in samples:
        raw, labels, mask = sample["raw"], sample["labels"], sample.get("mask")
        if not os.path.exists(raw):
            raise ValueError(f"Raw dataset path {raw} does not exist")
        if ".zarray" not in os.listdir(raw):
            raise ValueError(f"Raw dataset path {raw} does not contain a zarr array")
        if not os.path.exists(labels):
            raise ValueError(f"Labels dataset path {labels} does not exist")
        if ".zarray" not in os.listdir(labels) and not glob.glob(os.path.join(labels, "**", ".zarray"), recursive=True):
            raise ValueError(f"Labels dataset prefix {labels} does not contain any array")
        if mask is not None and not os.path.exists(mask):
            raise ValueError(f"Mask dataset path {mask} does not exist")
    return config


def affinity_targets(labels, unlabelled, neighborhood, grow_steps=0, only_xy=True, clip=(0.05, 0.95)):
    """models/3d_affs/train.py:127-139 on the device (bsmi_train_affinity_targets): GrowBoundary(labels,
    mask=unlabelled, steps, only_xy) -> AddAffinities(neighborhood) -> BalanceLabels.
    labels: int64 CUDA (D, H, W), overwritten with the grown-boundary labels; unlabelled: uint8 CUDA (D, H, W) or None.
    Returns (gt_affs, affs_weights), float32 (n, D, H, W)."""
    if labels.dtype != torch.int64 or not labels.is_cuda or not labels.is_contiguous():
        raise ValueError("labels must be a contiguous int64 CUDA tensor")
    if unlabelled is not None and (unlabelled.dtype != torch.uint8 or unlabelled.shape != labels.shape or not unlabelled.is_contiguous()):
        raise ValueError("unlabelled must be a contiguous uint8 tensor of the labels' shape")
    n = len(neighborhood)
    nb = (C.c_int32 * (3 * n))(*[int(v) for off in neighborhood for v in off])
    affs = torch.empty((n,) + tuple(labels.shape), dtype=torch.float32, device=labels.device)
    weights = torch.empty_like(affs)
    _lib.check(_lib.lib.bsmi_train_affinity_targets(
        labels.device.index, C.c_void_p(labels.data_ptr()), C.c_void_p(unlabelled.data_ptr()) if unlabelled is not None else None,
        _lib.i64x3(labels.shape), nb, n, int(grow_steps), 1 if only_xy else 0, float(clip[0]), float(clip[1]),
        C.c_void_p(affs.data_ptr()), C.c_void_p(weights.data_ptr()), C.c_void_p(torch.cuda.current_stream(labels.device).cuda_stream)))
    return affs, weights


def lsd_targets(labels, roi_offset, roi_shape, sigma, voxel_size, downsample=1, unlabelled=None):
    """3-D local shape descriptors of one sample on the device (reference models/3d_mtlsd/train.py:134-141).
    labels: int64 CUDA (D, H, W) holding the crop with the window context; -> (gt_lsds, lsds_weights) float32 (10, d, h, w)."""
    if labels.dtype != torch.int64 or not labels.is_cuda or labels.dim() != 3 or not labels.is_contiguous():
        raise ValueError("labels must be a contiguous int64 CUDA tensor")
    if unlabelled is not None and (unlabelled.dtype != torch.uint8 or unlabelled.shape != labels.shape or not unlabelled.is_contiguous()):
        raise ValueError("unlabelled must be a contiguous uint8 tensor of the labels' shape")
    sig = [float(sigma)] * 3 if isinstance(sigma, (int, float)) else [float(v) for v in sigma]
    out = torch.empty((10,) + tuple(int(v) for v in roi_shape), dtype=torch.float32, device=labels.device)
    weights = torch.empty_like(out)
    _lib.check(_lib.lib.bsmi_train_lsd_targets(
        labels.device.index, C.c_void_p(labels.data_ptr()), C.c_void_p(unlabelled.data_ptr()) if unlabelled is not None else None,
        _lib.i64x3(labels.shape), _lib.i64x3(roi_offset), _lib.i64x3(roi_shape), (C.c_float * 3)(*sig),
        (C.c_float * 3)(*[float(v) for v in voxel_size]), int(downsample), C.c_void_p(out.data_ptr()), C.c_void_p(weights.data_ptr()),
        C.c_void_p(torch.cuda.current_stream(labels.device).cuda_stream)))
    return out, weights


def lsd2d_targets(labels, roi_offset, roi_shape, sigma, voxel_size, downsample=1, unlabelled=None):
    """2-D local shape descriptors of a stack of sections in one launch (reference models/2d_mtlsd/train.py: Add2DLSDs).
    labels: int64 CUDA (S, H, W) holding the sections with the window context; roi_offset / roi_shape: (y, x);
    sigma / voxel_size: (y, x) world units.  -> (gt_lsds, lsds_weights) float32 (6, S, h, w)."""
    if labels.dtype != torch.int64 or not labels.is_cuda or labels.dim() != 3 or not labels.is_contiguous():
        raise ValueError("labels must be a contiguous int64 CUDA tensor (S, H, W)")
    if unlabelled is not None and (unlabelled.dtype != torch.uint8 or unlabelled.shape != labels.shape or not unlabelled.is_contiguous()):
        raise ValueError("unlabelled must be a contiguous uint8 tensor of the labels' shape")
    sig = [float(sigma)] * 2 if isinstance(sigma, (int, float)) else [float(v) for v in sigma]
    n = int(labels.shape[0])
    out = torch.empty((6, n) + tuple(int(v) for v in roi_shape), dtype=torch.float32, device=labels.device)
    weights = torch.empty_like(out)
    _lib.check(_lib.lib.bsmi_train_lsd2d_targets(
        labels.device.index, C.c_void_p(labels.data_ptr()), C.c_void_p(unlabelled.data_ptr()) if unlabelled is not None else None, n,
        (C.c_int64 * 2)(*labels.shape[1:]), (C.c_int64 * 2)(*[int(v) for v in roi_offset]), (C.c_int64 * 2)(*[int(v) for v in roi_shape]),
        (C.c_float * 2)(*sig), (C.c_float * 2)(*[float(v) for v in voxel_size]), int(downsample), C.c_void_p(out.data_ptr()),
        C.c_void_p(weights.data_ptr()), C.c_void_p(torch.cuda.current_stream(labels.device).cuda_stream)))
    return out, weights


def affinity_targets_roi(labels, unlabelled, roi_offset, roi_shape, neighborhood, grow_steps=0, only_xy=True, clip=(0.05, 0.95)):
    """GrowBoundary -> AddAffinities -> BalanceLabels of S independent label arrays that carry the neighbourhood's context
    (bsmi_train_affinity_targets_roi): affinities of the ROI only, balanced per array over its ROI.
    labels: int64 CUDA (S, D, H, W), overwritten with the grown-boundary labels; unlabelled: uint8 CUDA of that shape or None;
    roi_offset / roi_shape: (z, y, x).  Returns (gt_affs, affs_weights), float32 (n, S, d, h, w)."""
    if labels.dtype != torch.int64 or not labels.is_cuda or labels.dim() != 4 or not labels.is_contiguous():
        raise ValueError("labels must be a contiguous int64 CUDA tensor (S, D, H, W)")
    if unlabelled is not None and (unlabelled.dtype != torch.uint8 or unlabelled.shape != labels.shape or not unlabelled.is_contiguous()):
        raise ValueError("unlabelled must be a contiguous uint8 tensor of the labels' shape")
    n = len(neighborhood)
    nb = (C.c_int32 * (3 * n))(*[int(v) for off in neighborhood for v in off])
    s = int(labels.shape[0])
    affs = torch.empty((n, s) + tuple(int(v) for v in roi_shape), dtype=torch.float32, device=labels.device)
    weights = torch.empty_like(affs)
    _lib.check(_lib.lib.bsmi_train_affinity_targets_roi(
        labels.device.index, C.c_void_p(labels.data_ptr()), C.c_void_p(unlabelled.data_ptr()) if unlabelled is not None else None, s,
        _lib.i64x3(labels.shape[1:]), _lib.i64x3(roi_offset), _lib.i64x3(roi_shape), nb, n, int(grow_steps), 1 if only_xy else 0,
        float(clip[0]), float(clip[1]), C.c_void_p(affs.data_ptr()), C.c_void_p(weights.data_ptr()),
        C.c_void_p(torch.cuda.current_stream(labels.device).cuda_stream)))
    return affs, weights


def mask_sat(mask):
    """Summed-area table of mask sections on the device (bsmi_train_mask_sat): mask uint8 CUDA (S, H, W) -> int32 CUDA
    (S, H + 1, W + 1) holding the u32 counts (a section of fewer than 2^31 voxels keeps them non-negative)."""
    if mask.dtype != torch.uint8 or not mask.is_cuda or mask.dim() != 3 or not mask.is_contiguous():
        raise ValueError("mask must be a contiguous uint8 CUDA tensor (S, H, W)")
    s, h, w = (int(v) for v in mask.shape)
    sat = torch.empty((s, h + 1, w + 1), dtype=torch.int32, device=mask.device)
    _lib.check(_lib.lib.bsmi_train_mask_sat(mask.device.index, C.c_void_p(mask.data_ptr()), s, h, w, C.c_void_p(sat.data_ptr()),
                                            C.c_void_p(torch.cuda.current_stream(mask.device).cuda_stream)))
    return sat


def _read_world(ds, world_lo, shape, dtype):
    """ds[world_lo : world_lo + shape voxels] on ds's grid (world_lo in world units), zeros beyond the array (gp.Pad(x, None))."""
    vs, off = list(ds.voxel_size), list(ds.offset)
    nd = len(vs)
    lo = []
    for w, o, v in zip(world_lo, off, vs):
        if (w - o) % v:
            raise ValueError(f"{ds.path if hasattr(ds, 'path') else 'dataset'}: position {world_lo} is not on its voxel grid (offset {off}, voxel size {vs})")
        lo.append((w - o) // v)
    out = np.zeros(shape, dtype=dtype)
    full = ds.shape[-nd:]
    src, dst = [], []
    for a, n, m in zip(lo, shape, full):
        b0, b1 = max(a, 0), min(a + n, m)
        if b1 <= b0:
            return out
        src.append(slice(b0, b1))
        dst.append(slice(b0 - a, b1 - a))
    out[tuple(dst)] = ds[tuple(src)]
    return out


class SectionSource:
    """Infinite iterator of reference-style batches of the 2-D setups (models/2d_mtlsd/train.py:29-164, 2d_lsd, 2d_affs):
    `batch_size` independent draws of one output section each, stacked along the depth axis the training step reads.

    A draw picks a sample, then (z, y, x) of its output window inside the labels volume (one Generator, seed 42 + rank), and is
    rejected until at least 5 % of the window is known (gp.Reject(mask=unlabelled, min_masked=0.05); unlabelled = the mask
    dataset, else labels > 0).  The test is four lookups in a summed-area table of the mask, built on the device once per
    sample; only the sections that hold an acceptable window keep theirs (as uint32 on the host), so a store with one painted
    section in a hundred costs a hundredth of its voxels, and the draw loop never gives up while a window exists.
    Raw and mask are read at the labels' world position (their own offsets: ArraySource + MergeProvider), zeros beyond them.
    Batch: raw (in_channels * adj_slices, S, H, W) normalised to [-1, 1]; gt_lsds / lsds_weights (6, S, h, w);
    gt_affs / affs_weights (K, S, h, w)."""

    def __init__(self, samples, input_shape, output_shape, adj_slices=1, device=0, seed=42, batch_size=10, lsds=None, affs=None,
                 augment=None):
        """lsds: {"sigma", "downsample"} of net_config outputs.2d_lsds, or None; affs: {"neighborhood" (2-D offsets),
        "grow_boundary"} of outputs.2d_affs, or None.  augment: an augment2d.Aug2DParams (or True for the reference's
        arguments) turns on the geometric chain SimpleAugment -> DeformAugment -> ShiftAugment of every draw (augment2d.py),
        and with its field `intensity` set the intensity chain of raw after it, batched over the draws; None: un-augmented
        windows, the same batches as without the argument."""
        if lsds is None and affs is None:
            raise ValueError("a 2-D setup has a 2d_lsds and / or a 2d_affs output")
        self.augment = None
        if augment is not None and augment is not False:
            from . import augment2d as aug
            self.augment = aug.Aug2DParams() if augment is True else augment
            # refusals before any dataset is opened: a swap of non-square sections, a window that is not centred
            if self.augment.simple:
                aug.check_square(tuple(input_shape), tuple(output_shape))
            if any((int(i) - int(o)) % 2 for i, o in zip(input_shape, output_shape)):
                raise ValueError(f"augment2d: input_shape {list(input_shape)} - output_shape {list(output_shape)} must be even on every axis")
        self.samples = [(open_ds(s["raw"]), open_ds(s["labels"]), open_ds(s["mask"]) if s.get("mask") else None) for s in samples]
        self.inp, self.out = tuple(int(v) for v in input_shape), tuple(int(v) for v in output_shape)
        self.adj = int(adj_slices)
        self.dev = torch.device("cuda", device)
        self.rng = np.random.default_rng(seed)
        self.batch_size = int(batch_size)
        self.lsds, self.affs = lsds, affs
        self.ctx = [(i - o) // 2 for i, o in zip(self.inp, self.out)]
        lo, hi = [0, 0], [0, 0]
        if lsds is not None:
            self.df = int(lsds.get("downsample", 1))
            sig = lsds["sigma"]
            self.sigma = [float(sig)] * 2 if isinstance(sig, (int, float)) else [float(v) for v in sig]
            if any(o % self.df for o in self.out):
                raise ValueError(f"output_shape {list(self.out)} must be a multiple of the LSD downsample factor {self.df}")
        if affs is not None:
            self.nhood = [[0] + [int(v) for v in off] for off in affs["neighborhood"][: int(affs["dims"])]]
            self.grow = int(affs.get("grow_boundary", 0))
            # AddAffinities grows the labels request by the neighbourhood (negative offsets before, positive after)
            for d in range(2):
                lo[d] = max(0, -min(off[d + 1] for off in self.nhood))
                hi[d] = max(0, max(off[d + 1] for off in self.nhood))
        self.aff_lo, self.aff_hi = lo, hi
        self.vs = tuple(self.samples[0][1].voxel_size)
        for raw_ds, lab_ds, mask_ds in self.samples:
            if any(tuple(ds.voxel_size) != self.vs for ds in (raw_ds, lab_ds, mask_ds) if ds is not None):
                raise ValueError(f"raw, labels and mask of every sample must share one voxel size ({list(self.vs)})")
        # AddLocalShapeDescriptor.prepare: 3 sigma of context in y and x (sigma_z = 0), snapped to the sub-sampling grid
        self.lsd_ctx = [-(-int(-(-3.0 * s // v)) // self.df) * self.df for s, v in zip(self.sigma, self.vs[1:])] if lsds is not None else [0, 0]
        # one labels crop per draw serves both: the larger context on each side
        self.lo = [max(a, b) for a, b in zip(self.lsd_ctx, lo)]
        self.hi = [max(a, b) for a, b in zip(self.lsd_ctx, hi)]
        self.tables = [None] * len(self.samples)
        if self.augment is not None:
            from . import augment2d as aug
            # ... and before any read of data: a rotation on an anisotropic section grid (the voxel size is the stores' metadata)
            if self.augment.deform_p > 0 and self.augment.rotate:
                aug.check_rotation(self.vs)
            # the map is evaluated over the union of the input section and the labels window: the labels may reach beyond the input
            self.frame = aug.frame_of(self.inp, self.out, self.lo, self.hi)
            # prob_missing, where the config gives none, depends on adj_slices (models/2d_mtlsd/train.py:136)
            self.intensity = self.augment.intensity_for(self.adj)

    def _known(self, i, start, shape):
        """known-voxel mask (uint8) of the labels voxels [start, start + shape) of sample i, zeros beyond the volume"""
        _, lab_ds, mask_ds = self.samples[i]
        world = [o + a * v for o, a, v in zip(lab_ds.offset, start, lab_ds.voxel_size)]
        src = mask_ds if mask_ds is not None else lab_ds
        return (_read_world(src, world, tuple(shape), src.dtype) > 0).astype(np.uint8)

    def _tables(self, i):
        """{z: uint32 (H + 1, W + 1) summed-area table} of the sections of sample i that hold an acceptable window"""
        if self.tables[i] is None:
            _, lab_ds, mask_ds = self.samples[i]
            D, H, W = lab_ds.shape[-3:]
            h, w = self.out
            if H < h or W < w:
                raise ValueError("labels volume smaller than the network's output section")
            need = -(-5 * h * w // 100)   # >= 5 % of the window
            tables = {}
            step = max(1, min(D, (64 << 20) // max(1, H * W)))   # sections per device pass
            for z0 in range(0, D, step):
                nz = min(step, D - z0)
                m = torch.from_numpy(self._known(i, (z0, 0, 0), (nz, H, W))).to(self.dev)
                sat = mask_sat(m)
                totals = sat[:, H, W].cpu().numpy()
                for k in np.nonzero(totals >= need)[0]:
                    t = sat[int(k)].cpu().numpy().view(np.uint32).astype(np.int64)
                    win = t[h:, w:] - t[:-h, w:] - t[h:, :-w] + t[:-h, :-w]
                    if win.max() >= need:
                        tables[z0 + int(k)] = t.astype(np.uint32)
            self.tables[i] = tables
        return self.tables[i]

    def __iter__(self):
        return self

    def _draw(self):
        h, w = self.out
        need = -(-5 * h * w // 100)
        if not any(self._tables(i) for i in range(len(self.samples))):
            raise RuntimeError("no training location with at least 5 % labelled voxels in any sample")
        while True:
            i = int(self.rng.integers(len(self.samples)))
            shape = self.samples[i][1].shape[-3:]
            z, y, x = (int(self.rng.integers(0, s - o + 1)) for s, o in zip(shape, (1, h, w)))
            t = self._tables(i).get(z)
            if t is None:
                continue
            cnt = int(t[y + h, x + w]) - int(t[y, x + w]) - int(t[y + h, x]) + int(t[y, x])
            if cnt >= need:
                return i, z, y, x

    def _next_augmented(self):
        """One batch through the geometric chain.  Round 1 draws (location, plan) for the S slots in slot order -- the location
        by _draw(), then augment2d.draw_plan2d's order --, reads one box per draw (augment2d.source_box2d of the plan over the
        frame, zeros beyond the store) of raw (K sections), labels and mask, packs the S boxes, which differ in shape, into one
        staging buffer per array and uploads each once, then runs the four launches: coordinates, labels, mask, raw.  The 5 %
        test sees the augmented output window: one read-back of S counts after the mask launch decides which slots pass; the
        failing slots are drawn again in slot order, location and plan, and only they are run again.
        With augment2d.intensity, a round draws, after that read-back, one intensity plan (augment.draw_intensity_plan's order, for
        the stack (K, H, W)) for every slot it accepted, in slot order -- a rejected slot takes none of these draws --, its raw
        launch then writes the draws whose plan applies a node as v / 255, and after the last round ONE chain of batched launches
        (augment2d.apply_intensity2d) runs over the whole batch; a draw whose plan applies no node stays bit-equal."""
        from . import augment2d as aug
        S, K = self.batch_size, self.adj
        h, w = self.out
        H, W = self.inp
        lo, hi = self.lo, self.hi
        need = -(-5 * h * w // 100)
        window = ([c - l for c, l in zip(self.ctx, lo)], [h + lo[0] + hi[0], w + lo[1] + hi[1]])   # the labels window, in the input section's pixels
        raw_t = torch.empty((K, S, H, W), dtype=torch.float32, device=self.dev)
        lab_t = torch.empty((S, window[1][0], window[1][1]), dtype=torch.int64, device=self.dev)
        unl_t = torch.empty(lab_t.shape, dtype=torch.uint8, device=self.dev)
        slots = list(range(S))
        iplans, ipacked = [None] * S, None   # with augment2d.intensity: the accepted plan of every slot; the table of a round that filled the batch
        for _ in range(1000):
            plans, boxes, raws, labs, unls = [], [], [], [], []
            for _s in slots:
                i, z, y, x = self._draw()
                plan = aug.draw_plan2d(self.rng, self.augment, self.inp, self.frame, K, self.vs)
                box = aug.source_box2d(plan)
                raw_ds, lab_ds, _ = self.samples[i]
                vs, off = lab_ds.voxel_size, lab_ds.offset
                size = (box[1][0] - box[0][0], box[1][1] - box[0][1])
                # the box's origin in voxels of the labels volume: the input section starts ctx before the output window
                start = (z, y - self.ctx[0] + box[0][0], x - self.ctx[1] + box[0][1])
                world = [off[0] + (z - K // 2) * vs[0], off[1] + start[1] * vs[1], off[2] + start[2] * vs[2]]
                raws.append(_read_world(raw_ds, world, (K,) + size, np.uint8))
                world = [o + a * v for o, a, v in zip(off, start, vs)]
                lab = _read_world(lab_ds, world, (1,) + size, lab_ds.dtype)[0]
                # uint64 ids reinterpreted, not converted: the same bits as astype(int64)
                labs.append(lab.view(np.int64) if lab.dtype == np.uint64 else lab.astype(np.int64, copy=False))
                unls.append(self._known(i, start, (1,) + size)[0])
                plans.append(plan)
                boxes.append(box)
            packed = aug.Packed2D(plans, boxes)
            coords = aug.coords2d(packed, self.dev)
            lab_r = aug.sample_labels2d(packed, coords, torch.from_numpy(packed.pack(labs, np.int64)).to(self.dev), window)
            unl_r = aug.sample_mask2d(packed, coords, torch.from_numpy(packed.pack(unls, np.uint8)).to(self.dev), window)
            # gp.Reject(mask=unlabelled, min_masked=0.05) on the augmented output window of every slot: the one read-back of the round
            counts = unl_r[:, lo[0]:lo[0] + h, lo[1]:lo[1] + w].sum(dim=(1, 2), dtype=torch.int64)
            if self.intensity is None:
                raw_r = aug.sample_raw2d(packed, coords, torch.from_numpy(packed.pack(raws, np.uint8)).to(self.dev), ((0, 0), (H, W)))
            ok = (counts >= need).cpu().numpy()
            if self.intensity is not None:
                from .augment import IntensityPlan, draw_intensity_plan
                # the intensity draws come after the test has accepted a slot: a rejected one takes none of them
                drawn = [draw_intensity_plan(self.rng, self.intensity, (K, H, W)) if good else IntensityPlan((K, H, W)) for good in ok]
                for s, good, ip in zip(slots, ok, drawn):
                    if good:
                        iplans[s] = ip
                ipacked = aug.PackedIntensity2D(drawn)
                raw_r = aug.sample_unit2d(packed, coords, torch.from_numpy(packed.pack(raws, np.uint8)).to(self.dev), ipacked, ((0, 0), (H, W)))
            if ok.all() and len(slots) == S:
                raw_t, lab_t, unl_t = raw_r, lab_r, unl_r
            else:
                keep = torch.from_numpy(np.nonzero(ok)[0]).to(self.dev)
                dst = torch.tensor([slots[j] for j in np.nonzero(ok)[0]], dtype=torch.int64, device=self.dev)
                raw_t.index_copy_(1, dst, raw_r.index_select(1, keep))
                lab_t.index_copy_(0, dst, lab_r.index_select(0, keep))
                unl_t.index_copy_(0, dst, unl_r.index_select(0, keep))
            slots = [s for s, good in zip(slots, ok) if not good]
            if not slots:
                if self.intensity is not None:
                    # the round's own table where one round filled the batch, else one of the plans the slots were accepted with
                    aug.apply_intensity2d(raw_t, ipacked if ipacked.S == S else aug.PackedIntensity2D(iplans))
                batch = {"raw": raw_t}
                batch.update(self._targets(lab_t, unl_t))
                return batch
        raise RuntimeError("no training location with at least 5 % labelled voxels found after augmentation")

    def __next__(self):
        if self.augment is not None:
            return self._next_augmented()
        draws = [self._draw() for _ in range(self.batch_size)]
        h, w = self.out
        H, W = self.inp
        lo, hi = self.lo, self.hi
        big = (1, h + lo[0] + hi[0], w + lo[1] + hi[1])
        raw = np.zeros((self.adj, len(draws), H, W), dtype=np.uint8)
        lab = np.zeros((len(draws),) + big[1:], dtype=np.int64)
        unl = np.zeros((len(draws),) + big[1:], dtype=np.uint8)
        for s, (i, z, y, x) in enumerate(draws):
            raw_ds, lab_ds, _ = self.samples[i]
            vs, off = lab_ds.voxel_size, lab_ds.offset
            # raw: the section and its neighbours with the network's context, at the labels' world position
            world = [off[0] + (z - self.adj // 2) * vs[0], off[1] + (y - self.ctx[0]) * vs[1], off[2] + (x - self.ctx[1]) * vs[2]]
            raw[:, s] = _read_world(raw_ds, world, (self.adj, H, W), np.uint8)
            start = (z, y - lo[0], x - lo[1])
            world = [o + a * v for o, a, v in zip(off, start, vs)]
            lab[s] = _read_world(lab_ds, world, big, lab_ds.dtype)[0].astype(np.int64)
            unl[s] = self._known(i, start, big)[0]
        batch = {"raw": torch.from_numpy(raw).to(self.dev).float() * (1.0 / 255.0) * 2.0 - 1.0}
        lab_t = torch.from_numpy(lab).to(self.dev)
        unl_t = torch.from_numpy(unl).to(self.dev)
        batch.update(self._targets(lab_t, unl_t))
        return batch

    def _targets(self, lab_t, unl_t):
        """the targets of a batch from its labels and known-voxel mask over the labels window (S, h + lo + hi, w + lo + hi)"""
        h, w = self.out
        lo = self.lo
        batch = {}
        if self.lsds is not None:
            c = self.lsd_ctx
            ys, xs = slice(lo[0] - c[0], lo[0] + h + c[0]), slice(lo[1] - c[1], lo[1] + w + c[1])
            lsds, lw = lsd2d_targets(lab_t[:, ys, xs].contiguous(), c, self.out, self.sigma, self.vs[1:], self.df, unl_t[:, ys, xs].contiguous())
            batch.update(gt_lsds=lsds, lsds_weights=lw)
        if self.affs is not None:
            a, b = self.aff_lo, self.aff_hi
            ys, xs = slice(lo[0] - a[0], lo[0] + h + b[0]), slice(lo[1] - a[1], lo[1] + w + b[1])
            affs, aw = affinity_targets_roi(lab_t[:, None, ys, xs].contiguous(), unl_t[:, None, ys, xs].contiguous(), (0, a[0], a[1]),
                                            (1, h, w), self.nhood, self.grow, only_xy=True)
            batch.update(gt_affs=affs[:, :, 0], affs_weights=aw[:, :, 0])
        return batch


class SampleSource:
    """Infinite iterator of reference-style batches from (raw, labels[, mask]) Zarr volumes."""

    def __init__(self, samples, input_shape, output_shape, neighborhood, device=0, seed=42, head="affs", grow_boundary=0,
                 lsd_sigma=None, lsd_downsample=1, voxel_size=(1, 1, 1), augment=None):
        """augment: an augment.AugParams (or True for the reference's arguments) turns on the geometric chain SimpleAugment ->
        DeformAugment -> ShiftAugment (augment.py), and with its field `intensity` set the intensity chain of raw after it;
        None: un-augmented crops, the same batches as without the argument."""
        self.samples = [(open_ds(s["raw"]), open_ds(s["labels"]), open_ds(s["mask"]) if s.get("mask") else None) for s in samples]
        self.inp, self.out = tuple(input_shape), tuple(output_shape)
        self.nhood = [list(map(int, o)) for o in neighborhood]
        self.rng = np.random.default_rng(seed)
        self.dev = torch.device("cuda", device)
        self.grow = int(grow_boundary)
        # head: "affs" (3d_affs), "lsds" (3d_lsd) or "mtlsd" (3d_mtlsd: both, models/3d_mtlsd/train.py:134-153)
        if head not in ("affs", "lsds", "mtlsd"):
            raise ValueError(f"unknown head {head!r}")
        self.head = head
        self.lsd_sigma, self.lsd_df = lsd_sigma, int(lsd_downsample)
        self.voxel_size = tuple(float(v) for v in voxel_size)
        if head != "affs" and lsd_sigma is None:
            raise ValueError("the LSD head needs net_config outputs.3d_lsds.sigma")
        self.augment = None
        if augment is not None and augment is not False:
            from . import augment as aug
            self.augment = aug.AugParams() if augment is True else augment
            # refusals before any read: a swap of non-square blocks, a rotation on an anisotropic section grid, an LSD
            # context that the coordinate volume (the input block) does not cover
            if self.augment.simple:
                aug.check_square(self.inp, self.out)
            if self.augment.deform_p > 0 and self.augment.rotate and self.voxel_size[1] != self.voxel_size[2]:
                raise NotImplementedError(f"rotation about z needs voxel_size[1] == voxel_size[2], not {list(self.voxel_size)}; set "
                                          "augment.rotate = false (full 3-D rotations are not built)")
            ctx = [(i - o) // 2 for i, o in zip(self.inp, self.out)]
            if any((i - o) % 2 for i, o in zip(self.inp, self.out)):
                raise ValueError(f"augment: input_shape {list(self.inp)} - output_shape {list(self.out)} must be even on every axis")
            if any(c > x for c, x in zip(self._lsd_context(), ctx)):
                raise ValueError(f"augment: the LSD context {self._lsd_context()} exceeds the network's context {ctx}; the labels are "
                                 "resampled through the coordinates of the input block")

    def _lsd_context(self):
        """voxels of labels the descriptors need beyond the output block: 3 sigma, snapped to the sub-sampling grid; 0 without an LSD head"""
        if self.head == "affs":
            return [0, 0, 0]
        sig = [float(self.lsd_sigma)] * 3 if isinstance(self.lsd_sigma, (int, float)) else list(self.lsd_sigma)
        return [-(-int(-(-3.0 * s // v)) // self.lsd_df) * self.lsd_df for s, v in zip(sig, self.voxel_size)]

    def __iter__(self):
        return self

    @staticmethod
    def _read_padded(ds, lo, shape, dtype):
        """ds[lo : lo + shape] in voxels of its last three axes, zeros beyond the volume (gp.Pad(x, None))"""
        out = np.zeros(shape, dtype=dtype)
        src, dst = [], []
        for a, n, m in zip(lo, shape, ds.shape[-3:]):
            b0, b1 = max(a, 0), min(a + n, m)
            if b1 <= b0:
                return out
            src.append(slice(b0, b1))
            dst.append(slice(b0 - a, b1 - a))
        out[tuple(dst)] = ds[tuple(src)]
        return out

    def _next_augmented(self):
        """One batch through the geometric chain: location and plan drawn from self.rng (location first, then
        augment.draw_plan's order), one crop of raw, labels and mask -- augment.source_box of the plan, zeros beyond the
        volume -- uploaded, one coordinate launch, one resampling launch per array, the usual targets on the augmented
        labels and mask.  The 5 % test sees the augmented output block; a failing draw is redrawn, location and plan.
        With augment.intensity, the accepted attempt then draws its intensity plan (augment.draw_intensity_plan's order) and
        raw runs through the intensity chain; a plan that applies no node takes today's resampling launch."""
        from . import augment as aug
        ctx = [(i - o) // 2 for i, o in zip(self.inp, self.out)]
        cv = self._lsd_context()
        for _ in range(1000):
            raw_ds, lab_ds, mask_ds = self.samples[self.rng.integers(len(self.samples))]
            shape = lab_ds.shape[-3:]
            if any(s < o for s, o in zip(shape, self.out)):
                raise ValueError("labels volume smaller than the network's output block")
            off = [int(self.rng.integers(0, s - o + 1)) for s, o in zip(shape, self.out)]
            plan = aug.draw_plan(self.rng, self.augment, self.inp, self.voxel_size)
            lo, hi = aug.source_box(plan)
            start = [a - c + l for a, c, l in zip(off, ctx, lo)]      # the crop's origin in voxels of the volume
            size = tuple(h - l for l, h in zip(lo, hi))
            coords = aug.coords(plan, lo, self.dev)
            # labels and mask over the output block grown by the LSD context, all from the one coordinate volume
            region = ([c - v for c, v in zip(ctx, cv)], [o + 2 * v for o, v in zip(self.out, cv)])
            lab_np = self._read_padded(lab_ds, start, size, lab_ds.dtype)
            # uint64 ids reinterpreted, not converted: the same bits as astype(int64) without a second copy of the crop
            lab_crop = torch.from_numpy(lab_np.view(np.int64) if lab_np.dtype == np.uint64 else lab_np.astype(np.int64, copy=False)).to(self.dev)
            big = aug.sample_labels(coords, lab_crop, region)
            if mask_ds is not None:
                mask_crop = torch.from_numpy((self._read_padded(mask_ds, start, size, mask_ds.dtype) > 0).astype(np.uint8)).to(self.dev)
                bun = aug.sample_mask(coords, mask_crop, region)
            else:
                bun = (big > 0).to(torch.uint8)
            inner = tuple(slice(v, v + o) for v, o in zip(cv, self.out))
            unl_dev = bun[inner].contiguous()
            if float(unl_dev.float().mean()) < 0.05:   # gp.Reject(mask=unlabelled, min_masked=0.05), on the augmented block
                continue
            raw_crop = torch.from_numpy(self._read_padded(raw_ds, start, size, np.uint8)).to(self.dev)
            # the intensity draws come after the test has accepted the attempt: a rejected one takes none of them
            iplan = aug.draw_intensity_plan(self.rng, self.augment.intensity, self.inp) if self.augment.intensity is not None else None
            batch = {"raw": aug.sample_raw_intensity(coords, raw_crop, iplan)}
            if self.head != "affs":
                sig = [float(self.lsd_sigma)] * 3 if isinstance(self.lsd_sigma, (int, float)) else list(self.lsd_sigma)
                lsds, lw = lsd_targets(big, cv, self.out, sig, self.voxel_size, self.lsd_df, bun)
                batch.update(gt_lsds=lsds, lsds_weights=lw)
            if self.head != "lsds":
                affs, weights = affinity_targets(big[inner].contiguous(), unl_dev, self.nhood, self.grow, only_xy=True)
                batch.update(gt_affs=affs, affs_weights=weights)
            return batch
        raise RuntimeError("no training location with at least 5 % labelled voxels found")

    def __next__(self):
        if self.augment is not None:
            return self._next_augmented()
        ctx = [(i - o) // 2 for i, o in zip(self.inp, self.out)]
        for _ in range(1000):
            raw_ds, lab_ds, mask_ds = self.samples[self.rng.integers(len(self.samples))]
            shape = lab_ds.shape[-3:]
            if any(s < o for s, o in zip(shape, self.out)):
                raise ValueError("labels volume smaller than the network's output block")
            off = [int(self.rng.integers(0, s - o + 1)) for s, o in zip(shape, self.out)]
            sl = tuple(slice(a, a + o) for a, o in zip(off, self.out))
            labels = lab_ds[sl].astype(np.int64)
            unl = (mask_ds[sl] > 0) if mask_ds is not None else (labels > 0)
            if unl.mean() < 0.05:  # gp.Reject(mask=unlabelled, min_masked=0.05)
                continue
            # raw with context; outside the volume: zeros (gp.Pad(raw, None))
            raw = np.zeros(self.inp, dtype=np.uint8)
            rshape = raw_ds.shape[-3:]
            src, dst = [], []
            for a, c, n, i in zip(off, ctx, rshape, self.inp):
                lo, hi = max(a - c, 0), min(a - c + i, n)
                src.append(slice(lo, hi))
                dst.append(slice(lo - (a - c), hi - (a - c)))
            raw[tuple(dst)] = raw_ds[tuple(src)]
            x = torch.from_numpy(raw).to(self.dev).float() * (1.0 / 255.0) * 2.0 - 1.0
            lab = torch.from_numpy(labels).to(self.dev)
            unl_dev = torch.from_numpy(unl.astype(np.uint8)).to(self.dev)
            batch = {"raw": x}
            if self.head != "affs":
                # descriptors see the labels 3 sigma beyond the output block (AddLocalShapeDescriptor grows its request by
                # that context; beyond the volume the padded labels are 0), snapped to the sub-sampling grid
                df = self.lsd_df
                sig = [float(self.lsd_sigma)] * 3 if isinstance(self.lsd_sigma, (int, float)) else list(self.lsd_sigma)
                cv = [int(-(-3.0 * s // v)) for s, v in zip(sig, self.voxel_size)]
                cv = [-(-c // df) * df for c in cv]
                big = np.zeros([o + 2 * c for o, c in zip(self.out, cv)], dtype=np.int64)
                bun = np.zeros(big.shape, dtype=np.uint8)
                src, dst = [], []
                for a, c, n, o in zip(off, cv, shape, self.out):
                    lo, hi = max(a - c, 0), min(a + o + c, n)
                    src.append(slice(lo, hi))
                    dst.append(slice(lo - (a - c), hi - (a - c)))
                big[tuple(dst)] = lab_ds[tuple(src)].astype(np.int64)
                bun[tuple(dst)] = (mask_ds[tuple(src)] > 0) if mask_ds is not None else (big[tuple(dst)] > 0)
                lsds, lw = lsd_targets(torch.from_numpy(big).to(self.dev), cv, self.out, sig, self.voxel_size, df,
                                       torch.from_numpy(bun).to(self.dev))
                batch.update(gt_lsds=lsds, lsds_weights=lw)
            if self.head != "lsds":
                affs, weights = affinity_targets(lab, unl_dev, self.nhood, self.grow, only_xy=True)
                batch.update(gt_affs=affs, affs_weights=weights)
            return batch
        raise RuntimeError("no training location with at least 5 % labelled voxels found")


class SyntheticSource:
    """Infinite iterator of batches of the second-stage setups (models/3d_affs_from_2d_mtlsd/train.py:27-142, _from_2d_lsd,
    _from_2d_affs, _from_3d_lsd), which read no data store: CreateLabels of `input_shape` -> CustomGrowBoundary(inputs'
    grow_boundary, only_xy) -> ObfuscateLabels -> the inputs a first-stage net would have predicted from the obfuscated
    labels (Add2DLSDs per section or AddLocalShapeDescriptor, AddAffinities on [0, dy, dx]; labels are 0 beyond the block:
    gp.Pad(labels, None)) -> GrowBoundary(outputs' grow_boundary) on the clean labels, their affinities and balance weights
    over the central `output_shape`.  All of it on the device (synth_labels.SynthEngine and the target calls above); the host
    draws come from one random.Random(seed) stream, so one seed gives one sequence of batches, bit for bit.
    Batch: raw (1, C, D, H, W) = the inputs concatenated in net_config["inputs"] order; gt_affs / affs_weights (K, d, h, w).

    input_augment: an augment_inputs.InputAugParams (or True for the reference's arguments) degrades every input array the way
    the reference's train.py does ("simulate noisy defected predictions": noise, intensity per channel and per section,
    smoothing per section, low contrast; augment_inputs.py, csrc/augment_inputs.hip), in place, after the
    batch is made.  Its plans come from a stream of their own, np.random.default_rng((seed, 1)), one plan per input array in
    net_config["inputs"] order: the random.Random(seed) stream is not touched, so gt_affs and affs_weights are those of the
    un-augmented source batch by batch, and so is raw where no node of a plan is applied.  None (the default): today's batches.

    label_augment: an augment_labels.LabelAugParams (or True for the reference's arguments) turns on SimpleAugment -> DeformAugment
    -> ShiftAugment of the labels, where the reference has them: directly behind CreateLabels, before CustomGrowBoundary and
    ObfuscateLabels, so the inputs and the targets are all made from the warped labels.  One coordinate map of the block and one
    nearest resampling (augment_labels.warp_labels: the launches of csrc/augment.hip; labels are 0 outside the block, DESIGN.md
    section 7o).  Its plans (augment.draw_plan's order) come from a stream of their own, np.random.default_rng((seed, 2)): the
    random.Random(seed) stream and the (seed, 1) stream are not touched.  None (the default): today's batches, bit for bit, with
    or without `input_augment`.

    NOT built (logged by run_training): without `label_augment` SimpleAugment, DeformAugment, ShiftAugment of the labels; without
    `input_augment` the Noise / Intensity / Smooth / Defect augmentations of the inputs; with both DefectAugment's missing, deformed
    and artifact sections, which are 0 or absent in the reference's call."""

    NOT_BUILT = ("SimpleAugment, DeformAugment and ShiftAugment of the labels; NoiseAugment, IntensityAugment, SmoothAugment and "
                 "DefectAugment of the inputs")
    NOT_BUILT_WITH_INPUT_AUGMENT = ("SimpleAugment, DeformAugment and ShiftAugment of the labels; DefectAugment's missing, deformed and "
                                    "artifact sections of the inputs (0 / absent in the reference's call)")
    NOT_BUILT_WITH_LABEL_AUGMENT = "NoiseAugment, IntensityAugment, SmoothAugment and DefectAugment of the inputs"
    NOT_BUILT_WITH_BOTH = "DefectAugment's missing, deformed and artifact sections of the inputs (0 / absent in the reference's call)"

    def __init__(self, net_config, voxel_size=(1, 1, 1), device=0, seed=42, input_augment=None, label_augment=None):
        from .synth_labels import anisotropy_range
        ins = net_config.get("inputs", {})
        keys = set(ins)
        if not keys or not (keys <= {"2d_lsds", "2d_affs"} or keys == {"3d_lsds"}):
            raise NotImplementedError(f"synthetic labels feed the inputs 2d_lsds / 2d_affs or 3d_lsds, not {sorted(keys)}")
        if set(net_config["outputs"]) != {"3d_affs"}:
            raise NotImplementedError(f"synthetic labels train a 3d_affs output, not {sorted(net_config['outputs'])}")
        self.inputs = [(k, dict(v)) for k, v in ins.items()]
        self.inp = tuple(int(v) for v in net_config["input_shape"])
        self.out = tuple(int(v) for v in net_config["output_shape"])
        self.vs = tuple(float(v) for v in voxel_size)
        self.aniso = anisotropy_range(voxel_size)
        out3d = net_config["outputs"]["3d_affs"]
        self.out_nhood = [[int(v) for v in off] for off in out3d["neighborhood"][: int(out3d["dims"])]]
        self.out_grow = int(out3d.get("grow_boundary", 0))
        # models/3d_affs_from_2d_mtlsd/train.py:51 takes the 2d_affs input's grow_boundary, the others their only input's
        self.in_grow = int((ins.get("2d_affs") or ins.get("2d_lsds") or ins.get("3d_lsds")).get("grow_boundary", 0))
        for key, spec in self.inputs:
            df = int(spec.get("downsample", 1))
            if key != "2d_affs" and any(v % df for v in (self.inp[1:] if key == "2d_lsds" else self.inp)):
                raise ValueError(f"input_shape {list(self.inp)} must be a multiple of the LSD downsample factor {df}")
        self.device = int(device)
        self.rng = random.Random(seed)
        self.engine = None   # made by the first batch: the constructor touches no GPU
        self.arrays, at = [], 0   # (input, first channel, channel after the last) of every input array inside raw
        for key, spec in self.inputs:
            self.arrays.append((key, at, at + int(spec["dims"])))
            at += int(spec["dims"])
        if input_augment is True:
            from .augment_inputs import InputAugParams
            input_augment = InputAugParams()
        self.input_augment = input_augment
        self.aug_rng = np.random.default_rng((int(seed), 1)) if input_augment is not None else None
        self.label_augment, self.label_params, self.label_rng = None, None, None
        if label_augment is not None and label_augment is not False:
            from .augment_labels import LabelAugParams, check_block
            self.label_augment = LabelAugParams() if label_augment is True else label_augment
            # refusals before any GPU work: a swap of a non-square block, a rotation on an anisotropic section grid, a control
            # lattice larger than the coordinate launch holds
            check_block(self.label_augment, self.inp, self.vs)
            self.label_params = self.label_augment.to_aug_params(self.vs)   # what augment.draw_plan takes
            self.label_rng = np.random.default_rng((int(seed), 2))

    def __iter__(self):
        return self

    def _engine(self):
        if self.engine is None:
            from .synth_labels import SynthEngine
            self.engine = SynthEngine((self.inp[0] * self.aniso[1], self.inp[1], self.inp[2]), self.device)
        return self.engine

    def labels(self):
        """(clean labels after the inputs' grow_boundary, obfuscated labels): int64 CUDA of input_shape.  The order is the
        reference's: create_labels -> the warp of `label_augment`, where set -> grow_boundary -> obfuscate."""
        from .synth_labels import draw_plan
        eng = self._engine()
        lab = eng.create_labels(draw_plan(self.rng, self.inp, self.aniso))
        if self.label_augment is not None:
            from . import augment
            from .augment_labels import warp_labels
            lab = warp_labels(lab, augment.draw_plan(self.label_rng, self.label_params, self.inp, self.vs))
        if self.in_grow > 0:
            lab = eng.grow_boundary(lab, self.rng.getrandbits(64), self.in_grow)
        return lab, eng.obfuscate(lab, self.rng)

    def _input(self, key, spec, obf):
        pad = torch.nn.functional.pad
        if key == "2d_affs":
            nhood = [[0] + [int(v) for v in off] for off in spec["neighborhood"][: int(spec["dims"])]]
            lo = [max(0, -min(off[d] for off in nhood)) for d in (1, 2)]
            hi = [max(0, max(off[d] for off in nhood)) for d in (1, 2)]
            big = pad(obf, (lo[1], hi[1], lo[0], hi[0]))
            return affinity_targets_roi(big[None].contiguous(), None, (0, lo[0], lo[1]), self.inp, nhood, 0, only_xy=True)[0][:, 0]
        df, sig = int(spec.get("downsample", 1)), float(spec["sigma"])
        if key == "2d_lsds":
            c = [-(-int(-(-3.0 * sig // v)) // df) * df for v in self.vs[1:]]   # as SectionSource: 3 sigma, on the sub-sampling grid
            big = pad(obf, (c[1], c[1], c[0], c[0]))
            return lsd2d_targets(big.contiguous(), c, self.inp[1:], [sig, sig], self.vs[1:], df)[0]
        c = [-(-int(-(-3.0 * sig // v)) // df) * df for v in self.vs]
        big = pad(obf, (c[2], c[2], c[1], c[1], c[0], c[0]))
        return lsd_targets(big.contiguous(), c, self.inp, sig, self.vs, df)[0]

    def __next__(self):
        lab, obf = self.labels()
        raw = torch.cat([self._input(key, spec, obf) for key, spec in self.inputs], dim=0)[None].contiguous()
        ctx = [(i - o) // 2 for i, o in zip(self.inp, self.out)]
        affs, weights = affinity_targets_roi(lab[None].contiguous(), None, ctx, self.out, self.out_nhood, self.out_grow, only_xy=True)
        if self.input_augment is not None:
            from .augment_inputs import apply_inputs, draw_input_plan
            if tuple(raw.shape[1:]) != (self.arrays[-1][2], *self.inp):
                raise RuntimeError(f"raw of shape {tuple(raw.shape)} does not hold the inputs' {self.arrays[-1][2]} channels of {self.inp}")
            for _, lo, hi in self.arrays:
                plan = draw_input_plan(self.aug_rng, self.input_augment, (hi - lo, *self.inp))
                if plan.applied:
                    apply_inputs(raw[0, lo:hi], plan)   # a contiguous channel range of the batch, changed in place
        return {"raw": raw, "gt_affs": affs[:, 0].contiguous(), "affs_weights": weights[:, 0].contiguous()}


class PrefetchSource:
    """Batches produced ahead of the training thread (reference training.py:107-114: `DataLoader(dataset, num_workers=8,
    persistent_workers=True, pin_memory=True)`): a producer thread walks `source` -- Zarr chunk decoding runs in libbsmi's
    native threads without the GIL, the target kernels on a side stream -- and keeps up to `depth` finished batches queued,
    so a 20 ms training step never waits for crops and targets.  One producer: the batches come in the source's own order
    (same seed, same sequence as the source used directly)."""

    def __init__(self, source, depth=4, device=0):
        import queue
        import threading
        self.source = source
        self.dev = torch.device("cuda", device)
        self.q = queue.Queue(maxsize=max(1, int(depth)))
        self.stream = torch.cuda.Stream(self.dev)
        self._stop = False
        self.thread = threading.Thread(target=self._run, name="bsmi-samples", daemon=True)
        self.thread.start()

    def _run(self):
        try:
            with torch.cuda.stream(self.stream):
                for batch in self.source:
                    ev = torch.cuda.Event()
                    ev.record(self.stream)
                    while not self._stop:
                        try:
                            self.q.put((batch, ev), timeout=0.1)
                            break
                        except Exception:  # noqa: BLE001 - queue.Full: the trainer is busy, try again
                            continue
                    if self._stop:
                        return
        except BaseException as exc:  # noqa: BLE001 - handed to the training thread
            self.q.put(exc)

    def __iter__(self):
        return self

    def __next__(self):
        item = self.q.get()
        if isinstance(item, BaseException):
            raise item
        batch, ev = item
        ev.synchronize()   # host-side: a stream parked behind a device-side wait slows the kernels that run meanwhile
        cur = torch.cuda.current_stream(self.dev)
        for t in batch.values():
            t.record_stream(cur)   # allocated on the producer's stream, used on the trainer's
        return batch

    def close(self):
        self._stop = True
        try:
            while True:
                self.q.get_nowait()
        except Exception:  # noqa: BLE001 - queue.Empty
            pass
        self.thread.join(timeout=5)


BATCH_2D = 10   # models/2d_*/train.py: batch_size = 10 sections per step (gp.Stack)


def setup_name(net_config):
    """The reference's setup directory name of a net_config: 2d_mtlsd, 3d_affs_from_2d_lsd, ..."""
    def name(keys):
        dim = "2d" if any(k.startswith("2d") for k in keys) else "3d"
        kinds = {k.split("_", 1)[1] for k in keys}
        return f"{dim}_" + ("mtlsd" if kinds == {"affs", "lsds"} else ("lsd" if kinds == {"lsds"} else "affs"))
    out = name(net_config["outputs"])
    if set(net_config.get("inputs", {"raw": None})) == {"raw"}:
        return out
    return f"{out}_from_{name(net_config['inputs'])}"


def training_settings(net_config):
    """What a training step of this setup is: {"two_d", "batch_size", "in_shape", "lr"}.  2-D setups train on a stack of
    BATCH_2D sections, (S, H, W) for the lifted net, with Adam at lr 1e-4 (models/2d_mtlsd/train.py:194, 2d_lsd:154,
    2d_affs:161); the 3-D ones on one block at 0.5e-4 (models/3d_affs/train.py)."""
    dfs = net_config["downsample_factors"]
    two_d = bool(dfs) and len(dfs[0]) == 2
    inp = [int(v) for v in net_config["input_shape"]]
    if two_d:
        return {"two_d": True, "batch_size": BATCH_2D, "in_shape": (BATCH_2D, *inp), "lr": 1.0e-4}
    return {"two_d": False, "batch_size": 1, "in_shape": tuple(inp), "lr": 0.5e-4}


def make_sample_source(config, net_config, device=0, rank=0):
    """The built-in sample stream of `bs train` for this rank: seed 42 + rank, so that data-parallel ranks see different
    samples (with one seed for all, the averaged gradient would be the single-rank gradient computed N times)."""
    outs = net_config["outputs"]
    from .augment import AugParams
    augment = AugParams.from_config(config.get("augment"))
    if augment is not None:
        if set(net_config.get("inputs", {"raw": None})) != {"raw"}:
            raise NotImplementedError(f"augment: not built for synthetic labels (SyntheticSource, the {setup_name(net_config)} setup); "
                                      "it covers 3d_affs, 3d_lsd and 3d_mtlsd")
        if outs and not set(outs) - {"2d_affs", "2d_lsds"}:
            raise NotImplementedError(f"augment: not built for the 2-D setups (SectionSource, {setup_name(net_config)}); "
                                      "it covers 3d_affs, 3d_lsd and 3d_mtlsd (the 2-D setups have the key `augment2d`)")
    from .augment2d import Aug2DParams
    augment2d = Aug2DParams.from_config(config.get("augment2d"))
    if augment2d is not None and (set(net_config.get("inputs", {"raw": None})) != {"raw"} or not outs or set(outs) - {"2d_affs", "2d_lsds"}):
        raise NotImplementedError(f"augment2d: not built for the {setup_name(net_config)} setup; it covers 2d_affs, 2d_lsd and 2d_mtlsd "
                                  "(the first-stage 3-D setups have the key `augment`)")
    from .augment_inputs import InputAugParams
    input_augment = InputAugParams.from_config(config.get("input_augment"))
    second_stage = set(net_config.get("inputs", {"raw": None})) != {"raw"}
    if input_augment is not None and not (second_stage and config.get("synthetic_labels", False)):
        raise NotImplementedError(f"input_augment: not built for the {setup_name(net_config)} setup" + ("" if second_stage else
                                  " (its raw has the keys `augment` and `augment2d` with `intensity` inside)") + "; it degrades the inputs "
                                  "of the second-stage setups (3d_affs_from_2d_lsd, _2d_affs, _2d_mtlsd, _3d_lsd) and goes together with "
                                  "`synthetic_labels = true`")
    from .augment_labels import LabelAugParams
    label_augment = LabelAugParams.from_config(config.get("label_augment"))
    if label_augment is not None and not (second_stage and config.get("synthetic_labels", False)):
        raise NotImplementedError(f"label_augment: not built for the {setup_name(net_config)} setup" + ("" if second_stage else
                                  " (its samples have the keys `augment` and `augment2d`)") + "; it warps the synthetic labels "
                                  "of the second-stage setups (3d_affs_from_2d_lsd, _2d_affs, _2d_mtlsd, _3d_lsd) and goes together with "
                                  "`synthetic_labels = true`")
    if second_stage:
        if not config.get("synthetic_labels", False):
            raise NotImplementedError(f"the {setup_name(net_config)} setup trains on synthetic labels (CreateLabels / ObfuscateLabels), which "
                                      "the built-in sample source makes only when the train config sets `synthetic_labels = true`; "
                                      "without it it feeds 2d_affs, 2d_lsd, 2d_mtlsd, 3d_affs, 3d_lsd and 3d_mtlsd")
        return SyntheticSource(net_config, config.get("voxel_size", (1, 1, 1)), device=device, seed=42 + int(rank), input_augment=input_augment,
                               label_augment=label_augment)
    if outs and not set(outs) - {"2d_affs", "2d_lsds"}:
        s = training_settings(net_config)
        return SectionSource(config["samples"], net_config["input_shape"], net_config["output_shape"], int(net_config.get("adj_slices", 1)),
                             device=device, seed=42 + int(rank), batch_size=s["batch_size"], lsds=outs.get("2d_lsds"), affs=outs.get("2d_affs"),
                             augment=augment2d)
    out3d, lsd3d = outs.get("3d_affs"), outs.get("3d_lsds")
    if set(outs) - {"3d_affs", "3d_lsds"} or not outs:
        raise NotImplementedError(f"the built-in sample source feeds the 2-D and 3-D setups, not the outputs {sorted(outs)}")
    head = "mtlsd" if out3d and lsd3d else ("affs" if out3d else "lsds")
    nhood = out3d["neighborhood"][: int(out3d["dims"])] if out3d else [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]
    return SampleSource(config["samples"], net_config["input_shape"], net_config["output_shape"], nhood, device=device,
                        seed=42 + int(rank), head=head, grow_boundary=int(out3d.get("grow_boundary", 0)) if out3d else 0,
                        lsd_sigma=lsd3d.get("sigma") if lsd3d else None, lsd_downsample=int(lsd3d.get("downsample", 1)) if lsd3d else 1,
                        voxel_size=config.get("voxel_size", (1, 1, 1)), augment=augment)


def default_init(net_config, seed=42):
    """torch's default Conv3d initialisation (kaiming_uniform(a=sqrt(5)), bias uniform(+-1/sqrt(fan_in))) for every
    parameter of the reference Model, keyed like its state_dict."""
    from .unet import HEAD_OF_OUTPUT, input_channels
    g = torch.Generator().manual_seed(seed)
    nf, inc = int(net_config["num_fmaps"]), int(net_config["fmap_inc_factor"])
    dfs = net_config["downsample_factors"]
    nl = len(dfs) + 1
    nd = len(dfs[0]) if dfs else 3   # 2-D setups: Conv2d (O, I, kh, kw) parameters, the first reading in_channels * adj_slices
    k3, one = [3] * nd, (1,) * nd
    ksd = net_config.get("kernel_size_down") or [[k3, k3]] * nl
    ksu = net_config.get("kernel_size_up") or [[k3, k3]] * (nl - 1)
    sd = {}

    def conv(key, cout, cin, k):
        fan_in = cin * int(np.prod(k))
        bound = 1.0 / np.sqrt(fan_in)
        sd[key + ".weight"] = ((torch.rand((cout, cin) + tuple(k), generator=g) * 2 - 1) * bound).numpy()
        sd[key + ".bias"] = ((torch.rand(cout, generator=g) * 2 - 1) * bound).numpy()

    def conv_pass(prefix, cin, cout, kernels):
        c = cin
        for i, k in enumerate(kernels):
            conv(f"{prefix}.conv_pass.{2 * i}", cout, c, k)
            c = cout
        conv(f"{prefix}.residual.0", cout, cin, one)

    for lvl in range(nl):
        conv_pass(f"unet.l_conv.{lvl}", input_channels(net_config) if lvl == 0 else nf * inc ** (lvl - 1), nf * inc ** lvl, ksd[lvl])
    nf_out = int(net_config.get("num_fmaps_out") or nf)   # second-stage nets: width of the last right-side ConvPass, read by the heads
    for lvl in range(nl - 1):
        conv_pass(f"unet.r_conv.0.{lvl}", nf * inc ** lvl + nf * inc ** (lvl + 1), nf_out if lvl == 0 else nf * inc ** lvl, ksu[lvl])
    for name, val in net_config["outputs"].items():
        conv_pass(HEAD_OF_OUTPUT[name], nf_out, int(val["dims"]), [one])
    return sd


def latest_checkpoint(setup_dir):
    ckpts = glob.glob(os.path.join(setup_dir, "model_checkpoint_*.ckpt"))
    if not ckpts:
        return None, 0
    step = lambda p: int(re.findall(r"(\d+)", os.path.basename(p))[-1])  # noqa: E731
    best = max(ckpts, key=step)
    return best, step(best)


def run_training(config_file, device=0, batches=None, log=print):
    """`bs train <config>`: returns the number of iterations run.  Under torch.distributed every rank draws its own
    samples (seed 42 + rank: Lightning's seed_everything(42, workers=True) gives each rank's loader workers their own
    stream, training.py:128) and the gradients are averaged over the ranks."""
    from .unet import Model
    from .training import Trainer, fit, load_optimizer_state
    dist = torch.distributed
    rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
    config = setup_train(config_file)
    setup_dir = config["setup_dir"]
    with open(os.path.join(setup_dir, "net_config.json")) as f:
        net_config = json.load(f)
    max_iterations = int(config["max_iterations"])
    model = Model(net_config, device=device, precision="f32")
    ckpt, done = latest_checkpoint(setup_dir)
    if ckpt:
        model.load_checkpoint(ckpt)
        log(f"resuming from {ckpt}")
    else:
        model.load_state_dict(default_init(net_config, seed=42))
    # `arithmetic`, `deterministic` (additions to the reference's train config): "split-bf16" (default) or "f32"; ordered
    # reductions so that two runs from the same state give the same bits (default false), see training.Trainer
    settings = training_settings(net_config)
    trainer = Trainer(model, settings["in_shape"], lr=settings["lr"], arithmetic=config.get("arithmetic", "split-bf16"),
                      deterministic=bool(config.get("deterministic", False)))
    if ckpt and load_optimizer_state(trainer, ckpt):
        log(f"optimizer state restored (step {trainer.step_count()})")
    if batches is None:
        if config.get("augment"):
            from .augment import NOT_BUILT, NOT_BUILT_WITH_INTENSITY, AugParams
            params = AugParams.from_config(config["augment"])
            if params.intensity is not None:
                log("note: geometric augmentation on the device (SimpleAugment, DeformAugment, ShiftAugment: `augment`) and the intensity "
                    "chain of raw (NoiseAugment, IntensityAugment, GammaAugment, ImpulseNoiseAugment, SmoothAugment, DefectAugment: "
                    f"`augment.intensity`); not built: {NOT_BUILT_WITH_INTENSITY}")
            else:
                log(f"note: geometric augmentation on the device (SimpleAugment, DeformAugment, ShiftAugment: `augment`); not built: {NOT_BUILT} "
                    "(`intensity = true` inside the `[augment]` table turns them on)")
        elif config.get("augment2d"):
            from .augment2d import INTENSITY_NODES, NOT_BUILT as NOT_BUILT_2D, Aug2DParams
            if Aug2DParams.from_config(config["augment2d"]).intensity is not None:
                log("note: geometric augmentation of the 2-D setups on the device (SimpleAugment, DeformAugment, ShiftAugment of every "
                    f"section of a batch: `augment2d`) and the intensity chain of raw ({INTENSITY_NODES}: `augment2d.intensity`), "
                    f"both batched over the draws of a step; not built: {NOT_BUILT_2D}")
            else:
                log("note: geometric augmentation of the 2-D setups on the device (SimpleAugment, DeformAugment, ShiftAugment of every "
                    f"section of a batch: `augment2d`); off: {INTENSITY_NODES} (`intensity = true` inside the `[augment2d]` table turns "
                    f"them on); not built: {NOT_BUILT_2D}")
        else:
            log("note: the reference's gunpowder augmentations are not part of this engine; samples are random crops "
                "(`augment = true` turns on the geometric chain of the 3-D setups, `augment2d = true` that of the 2-D setups)")
        batches = make_sample_source(config, net_config, device, rank)
        if isinstance(batches, SyntheticSource) and batches.label_augment is not None:
            from .augment_inputs import NODES
            if batches.input_augment is not None:
                log("note: synthetic labels (synthetic_labels = true) with the geometric augmentation of the labels (`label_augment`) and "
                    f"the input augmentation ({NODES}: `input_augment`) on the device; not built: {SyntheticSource.NOT_BUILT_WITH_BOTH}")
            else:
                log("note: synthetic labels (synthetic_labels = true) with the geometric augmentation of the labels on the device "
                    f"(`label_augment`); not built: {SyntheticSource.NOT_BUILT_WITH_LABEL_AUGMENT} (`input_augment = true` turns them on)")
        elif isinstance(batches, SyntheticSource) and batches.input_augment is not None:
            from .augment_inputs import NODES
            log(f"note: synthetic labels (synthetic_labels = true) with the input augmentation on the device ({NODES}: `input_augment`); "
                f"not built: {SyntheticSource.NOT_BUILT_WITH_INPUT_AUGMENT}")
        elif isinstance(batches, SyntheticSource):
            log(f"note: synthetic labels (synthetic_labels = true); not built: {SyntheticSource.NOT_BUILT}")
        depth = int(config.get("prefetch", 4))   # an addition to the reference's train config: batches kept ready (0: inline)
        if depth > 0:
            batches = PrefetchSource(batches, depth, device)
    try:
        n = fit(trainer, batches, max_iterations, int(config.get("save_checkpoints_every", 0)), setup_dir, log=log, start_iteration=done,
                save_snapshots_every=int(config.get("save_snapshots_every", 0)), voxel_size=config.get("voxel_size"))
    finally:
        if isinstance(batches, PrefetchSource):
            batches.close()
    trainer.close()
    return n
