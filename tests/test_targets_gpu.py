"""The training targets on the device (csrc/train_targets.hip, csrc/train2d.hip through the wrappers of train.py) against
their restatements, at the fixtures of tests/targets_cases.py: thin objects without a tap on the sub-sampled grid, labels
that differ only above bit 31, windows truncated by the array, cells of many labels, the largest LDS window, class fractions
beyond BalanceLabels' clip, sections of different regimes in one call, 3-D samples in one call, positive and mixed offsets,
no unlabelled mask, more ROI voxels than one pass of the grid.  tests/test_targets_cpu.py shows on the references alone that
every fixture has its property and that the gates used here refuse the faults they are meant for."""
import numpy as np
import pytest
import torch

import targets_cases as TC

pytestmark = pytest.mark.gpu


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()      # a copy: the fixtures are shared and read-only


@pytest.mark.parametrize("name", TC.LSD3D_NAMES)
def test_lsd_targets_cases(name):
    """bsmi_train_lsd_targets against oracle/lsd_ref.py: 1e-4 per channel, background exactly 0, weights bit-equal.
    `thin_origin`, `thin_offset` and `none` hold labelled voxels whose object has no tap in the window: there the offsets are
    minus the cell's position (0 after the clip, unless the cell is nearer the array origin than sigma)."""
    from bootstrapper_amd.train import lsd_targets
    c = TC.lsd_case(3, name)
    ref, wref = TC.lsd_reference(3, name)
    lsds, w = lsd_targets(_dev(c.labels), c.roi_offset, c.roi_shape, c.sigma, c.voxel_size, c.df, _dev(c.unl))
    got = lsds.cpu().numpy()
    print(f"3d-{name}: max abs error per channel", np.abs(got.astype(np.float64) - ref).max(axis=(1, 2, 3)))
    TC.gate_lsd(got, w.cpu().numpy(), ref, wref, c.labels[c.roi])


@pytest.mark.parametrize("name", TC.LSD2D_NAMES)
def test_lsd2d_targets_cases(name):
    """bsmi_train_lsd2d_targets against tests/lsd2d_ref.py, the same gates.  `rmax` is the launch with the most dynamic LDS
    the kernel accepts (r = 60: 149 420 B); `edge` and the `thin` cases fill the tile beyond the array with zeros; `df4` and
    `df8` walk cells of three and more labels on a grid of one whole tile by a whole and a partial one."""
    from bootstrapper_amd.train import lsd2d_targets
    c = TC.lsd_case(2, name)
    ref, wref = TC.lsd_reference(2, name)
    lsds, w = lsd2d_targets(_dev(c.labels), c.roi_offset, c.roi_shape, c.sigma, c.voxel_size, c.df, _dev(c.unl))
    got = lsds.cpu().numpy()
    print(f"2d-{name}: max abs error per channel", np.abs(got.astype(np.float64) - ref).max(axis=(1, 2, 3)))
    TC.gate_lsd(got, w.cpu().numpy(), ref, wref, c.labels[c.roi])


@pytest.mark.parametrize("name", TC.AFF_NAMES)
def test_affinity_targets_cases(name):
    """bsmi_train_affinity_targets against oracle/train_ref.py: grown labels and affinities bit-equal, balance weights to
    rtol 1e-6 and exactly 0 where the mask is 0."""
    from bootstrapper_amd.train import affinity_targets
    c = TC.aff_case(False, name)
    ref = TC.aff_reference(False, name)
    lab = _dev(c.labels)
    a, w = affinity_targets(lab, _dev(c.unl), c.nhood, c.steps, c.only_xy)
    assert tuple(a.shape) == (len(c.nhood),) + c.labels.shape
    TC.gate_affinity(lab.cpu().numpy(), a.cpu().numpy(), w.cpu().numpy(), ref)


@pytest.mark.parametrize("name", TC.AFF_ROI_NAMES)
def test_affinity_targets_roi_cases(name):
    """bsmi_train_affinity_targets_roi against oracle/train_ref.py on every sample on its own, cropped, with BalanceLabels
    restated on the crop of every sample; the same gates."""
    from bootstrapper_amd.train import affinity_targets_roi
    c = TC.aff_case(True, name)
    ref = TC.aff_reference(True, name)
    lab = _dev(c.labels)
    a, w = affinity_targets_roi(lab, _dev(c.unl), c.roi_offset, c.roi_shape, c.nhood, c.steps, c.only_xy)
    assert tuple(a.shape) == (len(c.nhood), c.labels.shape[0]) + tuple(c.roi_shape)
    TC.gate_affinity(lab.cpu().numpy(), a.cpu().numpy(), w.cpu().numpy(), ref)


@pytest.mark.parametrize("name", TC.SAT_NAMES)
def test_mask_sat_cases(name):
    from bootstrapper_amd.train import mask_sat
    m = TC.sat_case(name)
    TC.gate_sat(mask_sat(_dev(m)).cpu().numpy(), TC.sat_reference(m))
