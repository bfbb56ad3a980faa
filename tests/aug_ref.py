"""numpy restatement of the geometric training augmentation (bootstrapper_amd/augment.py, csrc/augment.hip, DESIGN.md
section 7j): the coordinate map in float64, sampling from a GIVEN coordinate field (nearest in float32 exactly as
specified, trilinear in float64), the gates of the comparisons, and a float32 emulation of the kernels into which the
CPU tests inject faults.

The gates are derived, not measured.  eps = 2^-24 is the unit roundoff of float32; every bound below is first order in eps
and multiplied by (1 + 2^-10) for the higher orders (fewer than 40 roundings: (1 + eps)^40 - 1 < 40 eps (1 + 2^-10)).
The plan holds the numbers the kernel reads (float32 matrix, lattice and 1 / spacing), so only the kernel's own arithmetic
is to be bounded.  A fused multiply-add rounds once where the bound counts two roundings, so contraction only helps.

coords, per axis a (before the swap, which carries the bound with the component):
  d = r - c                     exact: integers and half-integers below 2^20
  linear part                   one rounding per product, one for their sum, one for adding E:   eps (2 Q_a + |t_a|),
                                Q_a = sum_b |A_ab d_b|
  s = c_src +- t                one rounding:                                                    eps |s_a|
  E_a(r): lattice coordinate g_b = r_b * inv_sp_b + org, two roundings, eps 2 G_b with G_b = max |r_b| inv_sp_b + 1; the
          clamp is 1-Lipschitz and g - cell is exact (a float minus its own integer part or a neighbouring integer).  E is
          continuous and piecewise trilinear with slope at most 2 V_a per unit of g_b (V_a = max |lattice[a]|), so the error
          of g costs 4 eps V_a sum_b G_b whichever cell the rounded g falls in.  A lerp a + w (b - a) rounds three
          times: w (b - a) (d1 + d2) + l d3 <= 5 eps V_a; its inputs' errors pass through a convex combination.  Three
          levels: 15 eps V_a.
  gate_a(p) = eps (2 Q_a + |t_a| + |s_a| + V_a (15 + 4 sum_b G_b)) (1 + 2^-10)

raw, against the float64 trilinear on the same float32 coordinates (the weights s - floor(s) are then the same numbers):
  three lerp levels on values <= 255: 15 eps 255; (v * 2 - 255) / 255: v * 2 exact, the subtraction and the division one
  relative rounding each of a result of at most 1 in magnitude; in output units 30 eps + 2 eps.
  RAW_GATE = 32 eps (1 + 2^-10)
"""
import numpy as np

EPS = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
RAW_GATE = 32 * EPS * SLACK


def _grid(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


def elastic(plan, r, dtype=np.float64, clamp=True):
    """E(r): (3, D, H, W) trilinear interpolation of the plan's lattice at the positions r (list of 3 arrays)"""
    if plan.lattice is None:
        return np.zeros((3,) + r[0].shape, dtype=dtype)
    lat = plan.lattice.astype(dtype)
    n = lat.shape[1:]
    cell, w = [], []
    for a in range(3):
        org = dtype(1.0 if n[a] > 1 else 0.0)
        g = (r[a].astype(dtype) * dtype(plan.inv_spacing[a]) + org).astype(dtype)
        if clamp:
            g = np.clip(g, dtype(0), dtype(n[a] - 1))
        lo = np.minimum(np.floor(g).astype(np.int64), max(n[a] - 2, 0))
        if not clamp:   # the injected fault: indices wrap instead of stopping at the lattice
            lo = lo % n[a]
        cell.append((lo, np.minimum(lo + 1, n[a] - 1)))
        w.append((g - lo.astype(dtype)).astype(dtype))
    out = np.empty((3,) + r[0].shape, dtype=dtype)
    for a in range(3):
        v = lat[a]

        def lerp(p, q, f):
            return (p + f * (q - p)).astype(dtype)
        c = {}
        for iz in (0, 1):
            for iy in (0, 1):
                c[iz, iy] = lerp(v[cell[0][iz], cell[1][iy], cell[2][0]], v[cell[0][iz], cell[1][iy], cell[2][1]], w[2])
        out[a] = lerp(lerp(c[0, 0], c[0, 1], w[1]), lerp(c[1, 0], c[1, 1], w[1]), w[0])
    return out


def map_parts(plan, box_lo):
    """The map in float64 and what the gate needs: dict(s, t, q, g) with s (3, D, H, W) the source coordinate in voxels
    of the crop whose origin is box_lo, t and q (= Q_a) per component before swap and mirror, g = [G_z, G_y, G_x]."""
    shape = plan.shape
    z, y, x = _grid(shape)
    zi = z.astype(np.int64)
    r = [z, y, x]
    if plan.shifts is not None:
        r = [z, y + plan.shifts[0].astype(np.float64)[zi], x + plan.shifts[1].astype(np.float64)[zi]]
    c = [(n - 1) / 2.0 for n in shape]
    d = [r[a] - c[a] for a in range(3)]
    lin = plan.linear.astype(np.float64)
    e = elastic(plan, r)
    t = np.stack([lin[0] * d[0], lin[1] * d[1] + lin[2] * d[2], lin[3] * d[1] + lin[4] * d[2]]) + e
    q = np.stack([np.abs(lin[0] * d[0]), np.abs(lin[1] * d[1]) + np.abs(lin[2] * d[2]), np.abs(lin[3] * d[1]) + np.abs(lin[4] * d[2])])
    m = t[[0, 2, 1]] if plan.swap else t
    s = np.stack([(c[a] - box_lo[a]) + (-m[a] if plan.mirror[a] else m[a]) for a in range(3)])
    g = [float(np.abs(r[a]).max()) * float(plan.inv_spacing[a]) + 1.0 for a in range(3)] if plan.lattice is not None else [0.0] * 3
    return {"s": s, "t": t, "q": q, "g": g}


def map_f64(plan, box_lo):
    return map_parts(plan, box_lo)["s"]


def coords_gate(plan, box_lo, parts=None):
    """(3, D, H, W): the bound on |device - float64 map| per voxel and output axis, derived in the module docstring"""
    p = parts or map_parts(plan, box_lo)
    v = [float(np.abs(plan.lattice[a]).max()) for a in range(3)] if plan.lattice is not None else [0.0] * 3
    per = np.stack([2 * p["q"][a] + np.abs(p["t"][a]) + v[a] * (15 + 4 * sum(p["g"])) for a in range(3)])
    if plan.swap:
        per = per[[0, 2, 1]]
    return EPS * (per + np.abs(p["s"])) * SLACK


def _region(coords, region):
    if region is None:
        return coords
    (oz, oy, ox), (d, h, w) = region
    return coords[:, oz:oz + d, oy:oy + h, ox:ox + w]


def sample_nearest(coords, crop, region=None):
    """crop[clamp(floor(s + 1/2))] per axis, the sum and the floor in float32, exactly as specified"""
    s = _region(np.asarray(coords, dtype=np.float32), region)
    idx = []
    for a in range(3):
        i = np.floor(s[a] + np.float32(0.5))
        idx.append(np.clip(i, 0, crop.shape[a] - 1).astype(np.int64))
    return crop[idx[0], idx[1], idx[2]]


def trilinear_f64(coords, crop, region=None):
    """float64 trilinear interpolation of crop at the given coordinates, both corners of the cell clamped to the crop"""
    s = _region(np.asarray(coords), region).astype(np.float64)
    v = crop.astype(np.float64)
    lo, hi, w = [], [], []
    for a in range(3):
        b = np.floor(s[a])
        w.append(s[a] - b)
        b = b.astype(np.int64)
        lo.append(np.clip(b, 0, crop.shape[a] - 1))
        hi.append(np.clip(b + 1, 0, crop.shape[a] - 1))

    def lerp(p, q, f):
        return p + f * (q - p)
    c = {}
    for iz, zz in enumerate((lo[0], hi[0])):
        for iy, yy in enumerate((lo[1], hi[1])):
            c[iz, iy] = lerp(v[zz, yy, lo[2]], v[zz, yy, hi[2]], w[2])
    return lerp(lerp(c[0, 0], c[0, 1], w[1]), lerp(c[1, 0], c[1, 1], w[1]), w[0])


def sample_raw(coords, crop, region=None):
    """the float64 reference of bsmi_aug_sample_f32_u8: trilinear, then v * 2 / 255 - 1"""
    return trilinear_f64(coords, crop, region) * 2.0 / 255.0 - 1.0


def box_contains(lo, hi, s):
    """every coordinate of s (3, ...), given relative to the box origin `lo`, and its neighbour floor(s) + 1 lie in the box"""
    return all(s[a].min() >= 0 and np.floor(s[a].max()) + 1 <= hi[a] - lo[a] - 1 for a in range(3))


# ---- a float32 emulation of the kernels, with faults to inject (tests/test_aug_cpu.py) ----

FAULTS = ("swapped_yx", "mirror_about_half", "unclamped_lattice", "shift_wrong_section", "ctx_dropped")


def emulate_coords(plan, box_lo, fault=None):
    """aug_coords_kernel in numpy float32, operation by operation.  fault: one of FAULTS[:4] or None."""
    f32 = np.float32
    shape = plan.shape
    z, y, x = [g.astype(f32) for g in _grid(shape)]
    zi = z.astype(np.int64)
    r = [z, y, x]
    if plan.shifts is not None:
        zs = np.minimum(zi + 1, shape[0] - 1) if fault == "shift_wrong_section" else zi
        r = [z, (y + plan.shifts[0].astype(f32)[zs]).astype(f32), (x + plan.shifts[1].astype(f32)[zs]).astype(f32)]
    c = [f32((n - 1) / 2.0) for n in shape]
    d = [(r[a] - c[a]).astype(f32) for a in range(3)]
    lin = plan.linear.astype(f32)
    e = elastic(plan, r, dtype=f32, clamp=fault != "unclamped_lattice")
    t = [lin[0] * d[0] + e[0], (lin[1] * d[1] + lin[2] * d[2]) + e[1], (lin[3] * d[1] + lin[4] * d[2]) + e[2]]
    if fault == "swapped_yx":
        t = [t[0], (lin[1] * d[2] + lin[2] * d[1]) + e[1], (lin[3] * d[2] + lin[4] * d[1]) + e[2]]
    if plan.swap:
        t = [t[0], t[2], t[1]]
    out = np.empty((3,) + shape, dtype=f32)
    for a in range(3):
        src = f32(c[a] - f32(box_lo[a]))
        if plan.mirror[a] and fault == "mirror_about_half":
            src = f32(src + f32(0.5))   # mirrors about I / 2 instead of (I - 1) / 2
        out[a] = src + (-t[a] if plan.mirror[a] else t[a])
    return out


def emulate_labels(coords, crop, ctx, out_shape, fault=None):
    """aug_sample_nearest over the central output region of the coordinate volume; fault "ctx_dropped": region offset 0"""
    off = (0, 0, 0) if fault == "ctx_dropped" else tuple(ctx)
    return sample_nearest(coords, crop, (off, tuple(out_shape)))


# ---- the cases of tests/test_aug_gpu.py, built here so that tests/test_aug_cpu.py runs the same comparisons on the emulation ----

BLOCKS = {"5x24x24": (5, 24, 24), "3x17x33": (3, 17, 33), "1x20x20": (1, 20, 20)}   # the second: odd width, no multiple of a wave or a vector; the third: a one-node z lattice
SPACINGS = {"single_cell": None, "spacing4": 4.0}   # None: larger than the block on every axis


def build_plan(shape, spacing, seed):
    """A full plan -- mirrors, swap where the block is square, scaling, rotation, lattice, shifts -- from its own seeded
    stream (not draw_plan's: the kernels are tested on their inputs, whatever drew them).  spacing None: 1.5 x the largest
    axis, so the block lies in one cell; 4: with cumulative shifts of sigma 6 that push r beyond the lattice."""
    from bootstrapper_amd.augment import AugPlan, lattice_shape, linear_of
    rng = np.random.default_rng(seed)
    sp = [1.5 * max(shape)] * 3 if spacing is None else [float(spacing)] * 3
    n = lattice_shape(shape, sp)
    u, theta = float(rng.uniform(0.9, 1.1)), float(rng.uniform(0, 2 * np.pi))
    shifts = np.cumsum(np.rint(rng.normal(0, 6.0, (shape[0], 2))), axis=0).T
    if spacing is not None:
        shifts[:, 0] += (8, -9)   # beyond the one node of margin (4 voxels) on both sides across the block
    return AugPlan(shape, mirror=(True, False, True), swap=shape[1] == shape[2], u=u, theta=theta, linear=linear_of(u, theta),
                   lattice=(rng.standard_normal((3,) + n) * 2.0).astype(np.float32), inv_spacing=np.array([1.0 / v for v in sp], dtype=np.float32),
                   shifts=np.ascontiguousarray(shifts).astype(np.int32))


def build_crops(size, seed):
    """(raw uint8, labels int64, mask uint8) of `size`: noise, so that any wrong index shows"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, size, dtype=np.uint8), rng.integers(1, 2 ** 40, size, dtype=np.int64), rng.integers(0, 2, size, dtype=np.uint8))


def coords_excess(got, plan, box_lo):
    """max over voxels and axes of |got - float64 map| / gate (must be <= 1), and the largest absolute difference"""
    parts = map_parts(plan, box_lo)
    diff = np.abs(np.asarray(got, dtype=np.float64) - parts["s"])
    return float((diff / coords_gate(plan, box_lo, parts)).max()), float(diff.max())


# ---- the store of tests/test_train_aug_gpu.py and its alignment check ----

def boxes_volume(shape, side, seed=0):
    """(raw uint8, labels uint64): the volume tiled by boxes of `side` voxels per axis (clipped at the far faces), ids from 1 with
    every thirteenth box left 0; raw is constant per label: (id * 37) % 256"""
    grid = [-(-s // b) for s, b in zip(shape, side)]
    ids = np.arange(1, int(np.prod(grid)) + 1, dtype=np.uint64).reshape(grid)
    ids[ids % 13 == 0] = 0
    labels = ids
    for a in range(3):
        labels = np.repeat(labels, side[a], axis=a)
    labels = np.ascontiguousarray(labels[:shape[0], :shape[1], :shape[2]])
    return ((labels * 37) % 256).astype(np.uint8), labels


def alignment(raw, labels):
    """raw float (O) and labels (O) of one output block -> (share of voxels checked, largest |raw - value of the label|
    over them): the voxels whose 3 x 3 x 3 neighbourhood in `labels` is uniform and non-zero"""
    lab = np.asarray(labels).astype(np.int64)
    ok = np.zeros(lab.shape, dtype=bool)
    inner = tuple(slice(1, n - 1) for n in lab.shape)
    ok[inner] = lab[inner] > 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nb = lab[tuple(slice(1 + d, n - 1 + d) for d, n in zip((dz, dy, dx), lab.shape))]
                ok[inner] &= nb == lab[inner]
    want = ((lab * 37) % 256) * 2.0 / 255.0 - 1.0
    err = np.abs(np.asarray(raw, dtype=np.float64) - want)[ok]
    return float(ok.mean()), float(err.max()) if err.size else 0.0
