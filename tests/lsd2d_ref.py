"""Test helper: numpy / scipy restatement of the 2-D local shape descriptors the reference's 2-D setups train against
(models/2d_mtlsd/train.py: Add2DLSDs, gp/add_2d_lsds.py -> lsd.train.LsdExtractor in 2-D on every section).

**Parity unpinned**, as for the 3-D descriptors (oracle/lsd_ref.py): the lsd package is neither in the reference nor
installed, and no reference test holds vectors for it.  This follows its published algorithm with two axes: per object,
Gaussian-weighted (scipy gaussian_filter, mode "constant", truncate 3.0) count, mean coordinate and coordinate covariance of
the object's mask on the `downsample`-times sub-sampled section, upsampled by repetition and written where the object is;
then normalisation to [0, 1] and clipping.  6 channels: mean offset (y, x), variances (y, x), Pearson yx, size."""
import numpy as np
from scipy.ndimage import gaussian_filter


def lsd2d_section(labels, roi_offset, roi_shape, sigma, voxel_size, downsample=1):
    """labels: int [H][W] (with context); -> descriptors float64 [6][h][w]"""
    df = int(downsample)
    labels = np.asarray(labels)
    sigma = np.asarray(sigma, np.float64)
    vs = np.asarray(voxel_size, np.float64)
    sub = labels[::df, ::df]
    sub_vs = vs * df
    sub_sigma = sigma / sub_vs
    coords = np.array(np.meshgrid(*[np.arange(n, dtype=np.float64) * sub_vs[d] for d, n in enumerate(sub.shape)], indexing="ij"))
    sl = tuple(slice(o, o + s) for o, s in zip(roi_offset, roi_shape))
    sub_sl = tuple(slice(o // df, (o + s) // df) for o, s in zip(roi_offset, roi_shape))
    out = np.zeros((6,) + tuple(roi_shape), np.float64)

    def agg(a):
        return gaussian_filter(a, sigma=sub_sigma, mode="constant", cval=0.0, truncate=3.0)[sub_sl]

    def up(a):
        return np.repeat(np.repeat(a, df, axis=1), df, axis=2)
    for l in np.unique(labels[sl]):
        if l == 0:
            continue
        m = (sub == l).astype(np.float64)
        count = agg(m)
        n = count.copy()
        n[n == 0] = 1
        mc = coords * m
        mean = np.array([agg(mc[d]) for d in range(2)]) / n
        offset = mean - coords[(slice(None),) + sub_sl]
        pairs = [(0, 0), (1, 1), (0, 1)]
        cov = np.array([agg(mc[i] * coords[j]) for i, j in pairs]) / n
        cov -= np.array([mean[i] * mean[j] for i, j in pairs])
        var, pe = cov[:2].copy(), cov[2:].copy()
        var[var < 1e-3] = 1e-3
        pe[0] /= np.sqrt(var[0] * var[1])
        var /= (sigma ** 2)[:, None, None]
        d = up(np.concatenate([offset, var, pe, count[None]]))
        out += d * (labels[sl] == l)
    fg = labels[sl] != 0
    out[[0, 1]] = out[[0, 1]] / sigma[:, None, None] * 0.5 + 0.5
    out[4] = out[4] * 0.5 + 0.5
    out[[0, 1, 4]] *= fg
    return np.clip(out, 0.0, 1.0)


def lsd2d_targets(labels, roi_offset, roi_shape, sigma, voxel_size, downsample=1, unlabelled=None):
    """labels: int [S][H][W]; -> (descriptors float32 [6][S][h][w], weights float32 [6][S][h][w]):
    weights = (labels != 0) * unlabelled over the ROI, repeated over the channels."""
    labels = np.asarray(labels)
    sl = (slice(None),) + tuple(slice(o, o + s) for o, s in zip(roi_offset, roi_shape))
    out = np.stack([lsd2d_section(sec, roi_offset, roi_shape, sigma, voxel_size, downsample) for sec in labels], axis=1)
    mask = (labels[sl] != 0).astype(np.float32)
    if unlabelled is not None:
        mask = mask * (np.asarray(unlabelled)[sl] > 0)
    return out.astype(np.float32), np.repeat(mask[None], 6, axis=0).astype(np.float32)
