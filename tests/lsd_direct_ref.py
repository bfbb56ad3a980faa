"""Test helper: float64 restatement of the local shape descriptors, 2-D and 3-D, by direct summation.

It shares nothing with the scipy restatements (oracle/lsd_ref.py, tests/lsd2d_ref.py): no filter, no per-object pass over the
array, no absolute coordinates.  Per cell of the `downsample`-times sub-sampled grid it cuts the window out of the
sub-sampled labels, truncated by the array (taps beyond the array do not exist, which is what a constant-0 filter
boundary amounts to), and per label of the cell's voxels sums
    n = sum w [label == l],  mean = sum w u / n,  cov = sum w (u - mean)(u - mean)^T / n
over it, with u the world coordinates relative to the cell and w the product of the normalised 1-D Gaussians
(sigma in sub-grid points, radius int(3 sigma + 0.5)).  A label with no tap in the window (n == 0) gets the lsd package's
values: mean 0 in absolute coordinates of the array, an offset of minus the cell's position; covariance 0.
Channels as the device writes them: offsets / sigma * 0.5 + 0.5 | variances (floored at 1e-3) / sigma^2 | Pearson
coefficients * 0.5 + 0.5 (3-D: zy, zx, yx) | n; clipped to [0, 1]; background voxels are zero.

`fault` restates one way a kernel can be wrong, for the tests that show the gates refuse it:
  "count0_cell"     n == 0 takes mean 0 relative to the cell
  "edge_replicate"  taps beyond the array repeat the edge instead of not existing
  "second_label"    the second label of a cell is written with the first label's statistics
"""
import numpy as np

FAULTS = (None, "count0_cell", "edge_replicate", "second_label")


def gauss1d(sigma_points):
    """(radius, normalised weights [2 radius + 1]) of a Gaussian of `sigma_points` sub-grid points truncated at 3 sigma"""
    r = int(3.0 * sigma_points + 0.5)
    k = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-0.5 * k * k / (sigma_points * sigma_points))
    return r, g / g.sum()


def lsd_direct(labels, roi_offset, roi_shape, sigma, voxel_size, downsample=1, fault=None):
    """labels: int [H][W] or [D][H][W] (with whatever context it has); -> float64 [6 | 10][*roi_shape]"""
    assert fault in FAULTS
    labels = np.asarray(labels)
    nd = labels.ndim
    df = int(downsample)
    sigma = np.broadcast_to(np.asarray(sigma, np.float64), (nd,))
    step = np.asarray(voxel_size, np.float64) * df
    sub = labels[(slice(None, None, df),) * nd]
    kern = [gauss1d(sigma[i] / step[i]) for i in range(nd)]
    pairs = [(i, j) for i in range(nd) for j in range(i + 1, nd)]
    out = np.zeros((2 * nd + len(pairs) + 1,) + tuple(roi_shape), np.float64)
    lo = [o // df for o in roi_offset]
    for rel in np.ndindex(*[s // df for s in roi_shape]):
        c = [a + b for a, b in zip(lo, rel)]
        idx, wgt, u = [], [], []
        for i in range(nd):
            r, w = kern[i]
            k = np.arange(c[i] - r, c[i] + r + 1)
            if fault == "edge_replicate":
                idx.append(np.clip(k, 0, sub.shape[i] - 1))
            else:
                keep = (k >= 0) & (k < sub.shape[i])
                k, w = k[keep], w[keep]
                idx.append(k)
            wgt.append(w)
            u.append((k - c[i]) * step[i])
        win = sub[np.ix_(*idx)]
        w = wgt[0]
        for i in range(1, nd):
            w = np.multiply.outer(w, wgt[i])
        u = np.meshgrid(*u, indexing="ij", sparse=True)
        block = labels[tuple(slice(c[i] * df, (c[i] + 1) * df) for i in range(nd))]
        view = out[(slice(None),) + tuple(slice(c[i] * df - roi_offset[i], (c[i] + 1) * df - roi_offset[i]) for i in range(nd))]
        first = None
        for l in block.ravel()[np.sort(np.unique(block.ravel(), return_index=True)[1])]:   # labels in voxel order
            if l == 0:
                continue
            wm = w * (win == l)
            n = wm.sum()
            if n > 0:
                mean = [(wm * u[i]).sum() / n for i in range(nd)]
                d = [u[i] - mean[i] for i in range(nd)]
                var = [(wm * d[i] * d[i]).sum() / n for i in range(nd)]
                cov = [(wm * d[i] * d[j]).sum() / n for i, j in pairs]
            else:
                mean = [0.0 if fault == "count0_cell" else -c[i] * step[i] for i in range(nd)]
                var, cov = [0.0] * nd, [0.0] * len(pairs)
            var = [max(v, 1e-3) for v in var]
            vals = np.array([mean[i] / sigma[i] * 0.5 + 0.5 for i in range(nd)] + [var[i] / sigma[i] ** 2 for i in range(nd)]
                            + [cov[k] / np.sqrt(var[i] * var[j]) * 0.5 + 0.5 for k, (i, j) in enumerate(pairs)] + [n])
            if fault == "second_label" and first is not None:
                vals, first = first, None
            elif first is None:
                first = vals
            view[:, block == l] = np.clip(vals, 0.0, 1.0)[:, None]
    return out


def lsd_direct_sections(labels, roi_offset, roi_shape, sigma, voxel_size, downsample=1, fault=None):
    """labels: int [S][H][W]; -> float64 [6][S][h][w]"""
    return np.stack([lsd_direct(sec, roi_offset, roi_shape, sigma, voxel_size, downsample, fault) for sec in labels], axis=1)
