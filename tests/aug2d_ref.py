"""numpy restatement of the geometric augmentation of the 2-D setups (bootstrapper_amd/augment2d.py, csrc/augment2d.hip,
DESIGN.md section 7l): the coordinate map of one draw in float64 over its frame and all K sections, sampling from a GIVEN
coordinate field (nearest in float32 exactly as specified, bilinear in float64), the batch-level references the GPU test
compares with (they read the PLANS and the per-draw crops, never the descriptor table, so a packing fault shows), the gates,
and a float32 emulation of the kernels reading the packed table into which the CPU tests inject faults.

The gates are derived, not measured.  eps = 2^-24 is the unit roundoff of float32; every bound below is first order in eps
and multiplied by (1 + 2^-10) for the higher orders (fewer than 40 roundings: (1 + eps)^40 - 1 < 40 eps (1 + 2^-10)).
The plan holds the numbers the kernel reads (float32 matrix, lattice and 1 / spacing), so only the kernel's own arithmetic
is to be bounded.  A fused multiply-add rounds once where the bound counts two roundings, so contraction only helps.

coords, per axis a (before the swap, which carries the bound with the component):
  d = r - c                     exact: integers and half-integers below 2^20
  linear part                   one rounding per product, one for their sum, one for adding E:   eps (2 Q_a + |t_a|),
                                Q_a = sum_b |A_ab d_b|
  s = c_src +- t                one rounding:                                                    eps |s_a|
  E_a(r): lattice coordinate g_b = q_b * inv_sp_b + 1 with q = r - F_lo an exact integer: two roundings, eps 2 G_b with
          G_b = max |r_b - F_lo,b| inv_sp_b + 1; the clamp is 1-Lipschitz and g - cell is exact (a float minus its own integer
          part or a neighbouring integer).  E is continuous and piecewise bilinear with slope at most 2 V_a per unit of g_b
          (V_a = max |lattice[a]|), so the error of g costs 4 eps V_a (G_y + G_x) whichever cell the rounded g falls in.  A
          lerp a + w (b - a) rounds three times: w (b - a) (d1 + d2) + l d3 <= 5 eps V_a; its inputs' errors pass through a
          convex combination.  Two levels (x, then y): 10 eps V_a.
  gate_a = eps (2 Q_a + |t_a| + |s_a| + V_a (10 + 4 (G_y + G_x))) (1 + 2^-10)

raw, against the float64 bilinear on the same float32 coordinates (the weights s - floor(s) are then the same numbers):
  two lerp levels on values <= 255: 10 eps 255; (v * 2 - 255) / 255: v * 2 exact, the subtraction and the division one
  relative rounding each of a result of at most 1 in magnitude; in output units 20 eps + 2 eps.
  RAW_GATE = 22 eps (1 + 2^-10)
"""
import numpy as np

EPS = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
RAW_GATE = 22 * EPS * SLACK


def frame_grid(plan, dtype=np.float64):
    """(y, x) of every frame pixel in the input section's pixels, each (F_h, F_w)"""
    (ly, lx), (hy, hx) = plan.frame
    return np.meshgrid(np.arange(ly, hy, dtype=dtype), np.arange(lx, hx, dtype=dtype), indexing="ij")


def elastic(plan, r, dtype=np.float64, origin=None):
    """E(r): (2, ...) bilinear interpolation of the plan's lattice at the positions r (list of 2 arrays in the input section's
    pixels).  origin: where the lattice coordinate is measured from, F_lo by the rule (an injected fault passes (0, 0))."""
    if plan.lattice is None:
        return np.zeros((2,) + r[0].shape, dtype=dtype)
    lat = plan.lattice.astype(dtype)
    n = lat.shape[1:]
    org = plan.frame[0] if origin is None else origin
    cell, w = [], []
    for a in range(2):
        g = ((r[a].astype(dtype) - dtype(org[a])).astype(dtype) * dtype(plan.inv_spacing[a]) + dtype(1.0)).astype(dtype)
        g = np.clip(g, dtype(0), dtype(n[a] - 1))
        lo = np.minimum(np.floor(g).astype(np.int64), n[a] - 2)
        cell.append((lo, lo + 1))
        w.append((g - lo.astype(dtype)).astype(dtype))

    def lerp(p, q, f):
        return (p + f * (q - p)).astype(dtype)
    out = np.empty((2,) + r[0].shape, dtype=dtype)
    for a in range(2):
        v = lat[a]
        c0 = lerp(v[cell[0][0], cell[1][0]], v[cell[0][0], cell[1][1]], w[1])
        c1 = lerp(v[cell[0][1], cell[1][0]], v[cell[0][1], cell[1][1]], w[1])
        out[a] = lerp(c0, c1, w[0])
    return out


def map_parts(plan, box_lo):
    """The map of one draw in float64 and what the gate needs: dict(s, t, q, g) with s (K, 2, F_h, F_w) the source coordinate
    in pixels of the crop whose origin is box_lo (relative to the input section), t and q (= Q_a) per component before swap
    and mirror, g = [G_y, G_x]."""
    y, x = frame_grid(plan)
    c = [(n - 1) / 2.0 for n in plan.shape]
    lin = plan.linear.astype(np.float64)
    ss, ts, qs = [], [], []
    g = [0.0, 0.0]
    for k in range(plan.sections):
        sh = plan.shifts[:, k].astype(np.float64) if plan.shifts is not None else (0.0, 0.0)
        r = [y + sh[0], x + sh[1]]
        d = [r[a] - c[a] for a in range(2)]
        t = np.stack([lin[0] * d[0] + lin[1] * d[1], lin[2] * d[0] + lin[3] * d[1]]) + elastic(plan, r)
        q = np.stack([np.abs(lin[0] * d[0]) + np.abs(lin[1] * d[1]), np.abs(lin[2] * d[0]) + np.abs(lin[3] * d[1])])
        m = t[::-1] if plan.swap else t
        ss.append(np.stack([(c[a] - box_lo[a]) + (-m[a] if plan.mirror[a + 1] else m[a]) for a in range(2)]))
        ts.append(t)
        qs.append(q)
        if plan.lattice is not None:
            g = [max(g[a], float(np.abs(r[a] - plan.frame[0][a]).max()) * float(plan.inv_spacing[a]) + 1.0) for a in range(2)]
    return {"s": np.stack(ss), "t": np.stack(ts), "q": np.stack(qs), "g": g}


def map_f64(plan, box_lo):
    return map_parts(plan, box_lo)["s"]


def coords_gate(plan, box_lo, parts=None):
    """(K, 2, F_h, F_w): the bound on |device - float64 map| per pixel and output axis, derived in the module docstring"""
    p = parts or map_parts(plan, box_lo)
    v = [float(np.abs(plan.lattice[a]).max()) for a in range(2)] if plan.lattice is not None else [0.0, 0.0]
    per = np.stack([2 * p["q"][:, a] + np.abs(p["t"][:, a]) + v[a] * (10 + 4 * sum(p["g"])) for a in range(2)], axis=1)
    if plan.swap:
        per = per[:, ::-1]
    return EPS * (per + np.abs(p["s"])) * SLACK


def coords_excess(got, plan, box_lo):
    """max over pixels, sections and axes of |got - float64 map| / gate (must be <= 1), and the largest absolute difference"""
    parts = map_parts(plan, box_lo)
    diff = np.abs(np.asarray(got, dtype=np.float64) - parts["s"])
    return float((diff / coords_gate(plan, box_lo, parts)).max()), float(diff.max())


def _window(plane, plan, region):
    """the part of a coordinate field (2, F_h, F_w) over `region` ((offset, shape) in the input section's pixels; None: all)"""
    if region is None:
        return plane
    (oy, ox), (h, w) = region
    oy, ox = oy - plan.frame[0][0], ox - plan.frame[0][1]
    return plane[:, oy:oy + h, ox:ox + w]


def sample_nearest(plane, crop):
    """crop[clamp(floor(s + 1/2))] per axis, the sum and the floor in float32, exactly as specified; plane (2, h, w)"""
    s = np.asarray(plane, dtype=np.float32)
    idx = [np.clip(np.floor(s[a] + np.float32(0.5)), 0, crop.shape[a] - 1).astype(np.int64) for a in range(2)]
    return crop[idx[0], idx[1]]


def bilinear_f64(plane, crop):
    """float64 bilinear interpolation of crop (h, w) at the given coordinates, both corners of the cell clamped to the crop"""
    s = np.asarray(plane).astype(np.float64)
    v = crop.astype(np.float64)
    lo, hi, w = [], [], []
    for a in range(2):
        b = np.floor(s[a])
        w.append(s[a] - b)
        b = b.astype(np.int64)
        lo.append(np.clip(b, 0, crop.shape[a] - 1))
        hi.append(np.clip(b + 1, 0, crop.shape[a] - 1))
    c0 = v[lo[0], lo[1]] + w[1] * (v[lo[0], hi[1]] - v[lo[0], lo[1]])
    c1 = v[hi[0], lo[1]] + w[1] * (v[hi[0], hi[1]] - v[hi[0], lo[1]])
    return c0 + w[0] * (c1 - c0)


def ref_nearest(coords, plans, crops, region=None):
    """The batch's labels or mask from a given coordinate field (S, K, 2, F_h, F_w): draw s through section K // 2's
    coordinates from ITS crop (h_s, w_s) -> (S, h, w)"""
    return np.stack([sample_nearest(_window(coords[s, p.sections // 2], p, region), crops[s]) for s, p in enumerate(plans)])


def ref_raw(coords, plans, crops, region=None):
    """The batch's raw from a given coordinate field: section k of draw s through its own coordinates from section k_src of
    ITS crop (K, h_s, w_s), v * 2 / 255 - 1 -> float64 (K, S, h, w)"""
    out = []
    for k in range(plans[0].sections):
        out.append(np.stack([bilinear_f64(_window(coords[s, k], p, region), crops[s][p.sections - 1 - k if p.mirror[0] else k]) * 2.0 / 255.0 - 1.0
                             for s, p in enumerate(plans)]))
    return np.stack(out)


def box_contains(lo, hi, s):
    """every coordinate of s (..., 2, h, w), given relative to the box origin `lo`, and its neighbour floor(s) + 1 lie in the box"""
    return all(s[..., a, :, :].min() >= 0 and np.floor(s[..., a, :, :].max()) + 1 <= hi[a] - lo[a] - 1 for a in range(2))


# ---- a float32 emulation of the kernels reading the packed table, with faults to inject (tests/test_aug2d_cpu.py) ----

FAULTS = ("previous_descriptor", "crop_offset_of_draw_0", "z_mirror_ignored", "labels_shift_of_section_0", "lattice_from_input_origin")


def emulate_coords(plans, boxes, fault=None):
    """aug2d_coords_kernel in numpy float32, operation by operation -> (S, K, 2, F_h, F_w).  fault "previous_descriptor": draw
    s > 0 computes with draw s - 1's plan and box; "lattice_from_input_origin": g = r * inv_sp + 1."""
    f32 = np.float32
    out = []
    for s in range(len(plans)):
        j = max(s - 1, 0) if fault == "previous_descriptor" else s
        plan, lo = plans[j], boxes[j][0]
        y, x = frame_grid(plan, f32)
        c = [f32((n - 1) / 2.0) for n in plan.shape]
        lin = plan.linear.astype(f32)
        per = []
        for k in range(plan.sections):
            sh = plan.shifts[:, k].astype(f32) if plan.shifts is not None else (f32(0), f32(0))
            r = [(y + sh[0]).astype(f32), (x + sh[1]).astype(f32)]
            d = [(r[a] - c[a]).astype(f32) for a in range(2)]
            e = elastic(plan, r, f32, (0, 0) if fault == "lattice_from_input_origin" else None)
            t = [(lin[0] * d[0] + lin[1] * d[1]) + e[0], (lin[2] * d[0] + lin[3] * d[1]) + e[1]]
            if plan.swap:
                t = t[::-1]
            per.append(np.stack([f32(c[a] - f32(lo[a])) + (-t[a] if plan.mirror[a + 1] else t[a]) for a in range(2)]).astype(f32))
        out.append(np.stack(per))
    return np.stack(out)


def emulate_nearest(coords, plans, packed_crops, shapes, offsets, region=None, fault=None):
    """aug2d_sample_nearest_kernel on the packed crops (1-D, draw s of shapes[s] at pixel offsets[s]).  fault
    "crop_offset_of_draw_0": every draw reads at offsets[0]; "labels_shift_of_section_0": section 0's coordinates."""
    out = []
    for s, p in enumerate(plans):
        off = offsets[0] if fault == "crop_offset_of_draw_0" else offsets[s]
        h, w = shapes[s]
        flat = packed_crops[off:off + h * w]
        crop = np.resize(flat, (h, w)) if flat.size < h * w else flat.reshape(h, w)   # a wrong offset may run past the end: wrap, as wrong as any
        k = 0 if fault == "labels_shift_of_section_0" else p.sections // 2
        out.append(sample_nearest(_window(coords[s, k], p, region), crop))
    return np.stack(out)


def emulate_raw(coords, plans, packed_crops, shapes, offsets, region=None, fault=None):
    """aug2d_sample_f32_u8_kernel in numpy float32 on the packed crops (draw s: K sections at pixel K * offsets[s]) -> (K, S, h, w).
    fault "z_mirror_ignored": k_src = k; "crop_offset_of_draw_0"."""
    f32 = np.float32
    K = plans[0].sections
    out = np.empty((K, len(plans)) + _window(coords[0, 0], plans[0], region).shape[1:], dtype=f32)
    for s, p in enumerate(plans):
        off = (offsets[0] if fault == "crop_offset_of_draw_0" else offsets[s]) * K
        h, w = shapes[s]
        flat = packed_crops[off:off + K * h * w]
        crop = (np.resize(flat, (K, h, w)) if flat.size < K * h * w else flat.reshape(K, h, w)).astype(f32)
        for k in range(K):
            ks = K - 1 - k if (p.mirror[0] and fault != "z_mirror_ignored") else k
            sc = _window(coords[s, k], p, region).astype(f32)
            b = [np.floor(sc[a]) for a in range(2)]
            wt = [(sc[a] - b[a]).astype(f32) for a in range(2)]
            i0 = [np.clip(b[a].astype(np.int64), 0, (h, w)[a] - 1) for a in range(2)]
            i1 = [np.clip(b[a].astype(np.int64) + 1, 0, (h, w)[a] - 1) for a in range(2)]
            v = crop[ks]
            c0 = (v[i0[0], i0[1]] + wt[1] * (v[i0[0], i1[1]] - v[i0[0], i0[1]])).astype(f32)
            c1 = (v[i1[0], i0[1]] + wt[1] * (v[i1[0], i1[1]] - v[i1[0], i0[1]])).astype(f32)
            val = (c0 + wt[0] * (c1 - c0)).astype(f32)
            out[k, s] = ((val * f32(2) - f32(255)).astype(f32) / f32(255)).astype(f32)
    return out


# ---- the cases of tests/test_aug2d_gpu.py, built here so that tests/test_aug2d_cpu.py runs the same comparisons on the emulation ----

CASES = {   # input, output, label margins lo / hi, K, swap
    "24sq_K3": ((24, 24), (16, 16), (6, 6), (6, 6), 3, True),
    "24sq_K1": ((24, 24), (16, 16), (6, 6), (6, 6), 1, True),
    "17x33_K3": ((17, 33), (9, 25), (2, 0), (0, 2), 3, False),   # odd sizes, no multiple of a wave or a vector; the frame is the input section
}
SPACINGS = {"single_cell": None, "spacing4": 4.0}   # None: larger than the frame on every axis
S = 3


def build_case(case, spacing, seed=11):
    """(plans, boxes, window) of a case: S = 3 different plans from their own seeded stream (not draw_plan2d's: the kernels are
    tested on their inputs, whatever drew them) -- draw 0 a full plan (mirrors z and x, swap where the case allows, scaling,
    rotation, lattice, shifts), draw 1 the IDENTITY (no lattice, no shifts: a draw between two full ones that must not see
    their descriptors), draw 2 another full plan (mirror y, other lattice and shifts, no swap).  spacing None: 1.5 x the
    largest frame axis, so the frame lies in one cell; 4: with shifts of +9 / -9 pixels that push r beyond the one node of
    margin on both sides.  The boxes are source_box2d's, so the crops differ in shape; draw 2's is cut by 3 pixels on every
    side, smaller than the map's range: the clamp of the sampling kernels works.  window: the labels window as a region."""
    from bootstrapper_amd import augment2d as A
    inp, out, lo, hi, K, swap = CASES[case]
    frame = A.frame_of(inp, out, lo, hi)
    fshape = tuple(h - l for l, h in zip(*frame))
    rng = np.random.default_rng(seed)
    sp = [1.5 * max(fshape)] * 2 if spacing is None else [float(spacing)] * 2
    n = A.lattice_shape(frame, sp)

    def full(mirror, sw):
        u, theta = float(rng.uniform(0.9, 1.1)), float(rng.uniform(0, 2 * np.pi))
        shifts = np.rint(rng.normal(0, 2.0, (2, K)))
        shifts[0, 0], shifts[1, K - 1] = 9, -9
        return A.Aug2DPlan(inp, frame, K, mirror=mirror, swap=sw, u=u, theta=theta, linear=A.linear_of(u, theta),
                           lattice=(rng.standard_normal((2,) + n) * 2.0).astype(np.float32),
                           inv_spacing=np.array([1.0 / v for v in sp], dtype=np.float32), shifts=shifts.astype(np.int32))
    plans = [full((True, False, True), swap), A.Aug2DPlan(inp, frame, K), full((False, True, False), False)]
    boxes = [A.source_box2d(p) for p in plans]
    (l, h) = boxes[2]
    boxes[2] = (tuple(v + 3 for v in l), tuple(v - 3 for v in h))
    ctx = [(i - o) // 2 for i, o in zip(inp, out)]
    window = (tuple(c - m for c, m in zip(ctx, lo)), tuple(o + a + b for o, a, b in zip(out, lo, hi)))
    return plans, boxes, window


def build_crops(boxes, K, seed=12):
    """per draw (raw uint8 (K, h, w), labels int64 (h, w), mask uint8 (h, w)) of its box: noise, so that any wrong index shows"""
    rng = np.random.default_rng(seed)
    raw, lab, mask = [], [], []
    for lo, hi in boxes:
        size = (hi[0] - lo[0], hi[1] - lo[1])
        raw.append(rng.integers(0, 256, (K,) + size, dtype=np.uint8))
        lab.append(rng.integers(1, 2 ** 40, size, dtype=np.int64))
        mask.append(rng.integers(0, 2, size, dtype=np.uint8))
    return raw, lab, mask


def regions(plans, window):
    """what every case is sampled over: the whole frame, the input section, the labels window"""
    return [None, ((0, 0), plans[0].shape), window]


def compare(plans, boxes, crops, window, coords, outputs):
    """The comparisons of the GPU test, on whatever produced `coords` (S, K, 2, F_h, F_w) and `outputs` = [(raw, labels, mask)
    per region of regions(plans, window)] -- the device or the emulation.  -> dict: coords_excess (largest |coords - float64
    map| / gate over the draws), coords_worst, labels_equal, mask_equal (bit for bit against the restatement reading THESE
    coords), raw_err (largest |raw - float64 bilinear on these coords|).  A pass is coords_excess <= 1, both equal, raw_err <=
    RAW_GATE."""
    raw_c, lab_c, mask_c = crops
    res = {"coords_excess": 0.0, "coords_worst": 0.0, "labels_equal": True, "mask_equal": True, "raw_err": 0.0}
    for s, (p, (lo, _)) in enumerate(zip(plans, boxes)):
        excess, worst = coords_excess(coords[s], p, lo)
        res["coords_excess"], res["coords_worst"] = max(res["coords_excess"], excess), max(res["coords_worst"], worst)
    for region, (raw, lab, mask) in zip(regions(plans, window), outputs):
        res["labels_equal"] &= bool(np.array_equal(lab, ref_nearest(coords, plans, lab_c, region)))
        res["mask_equal"] &= bool(np.array_equal(mask, ref_nearest(coords, plans, mask_c, region)))
        res["raw_err"] = max(res["raw_err"], float(np.abs(np.asarray(raw, dtype=np.float64) - ref_raw(coords, plans, raw_c, region)).max()))
    return res


def passes(res):
    return res["coords_excess"] <= 1.0 and res["labels_equal"] and res["mask_equal"] and res["raw_err"] <= RAW_GATE


# ---- the store of tests/test_train2d_aug_gpu.py, its draws without a device, and its alignment check ----

def alignment(raw, labels):
    """raw float (S, h, w) -- the centre channel over the output window -- and labels (S, h, w) of one batch -> (share of the
    batch's pixels checked, largest |raw - value of the label| over them): the pixels whose 3 x 3 neighbourhood in `labels`
    is uniform and non-zero.  raw of the store is (id * 37) % 256 (aug_ref.boxes_volume)."""
    lab = np.asarray(labels).astype(np.int64)
    ok = np.zeros(lab.shape, dtype=bool)
    inner = (slice(None), slice(1, lab.shape[1] - 1), slice(1, lab.shape[2] - 1))
    ok[inner] = lab[inner] > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            nb = lab[:, 1 + dy:lab.shape[1] - 1 + dy, 1 + dx:lab.shape[2] - 1 + dx]
            ok[inner] &= nb == lab[inner]
    want = ((lab * 37) % 256) * 2.0 / 255.0 - 1.0
    err = np.abs(np.asarray(raw, dtype=np.float64) - want)[ok]
    return float(ok.mean()), float(err.max()) if err.size else 0.0


def read_padded(vol, start, size):
    """vol[start : start + size], zeros beyond the volume"""
    out = np.zeros(size, dtype=vol.dtype)
    src = tuple(slice(max(a, 0), min(a + n, m)) for a, n, m in zip(start, size, vol.shape))
    if any(s.stop <= s.start for s in src):
        return out
    out[tuple(slice(s.start - a, s.stop - a) for s, a in zip(src, start))] = vol[src]
    return out


def simulate_batches(raw, labels, params, inp, out, lo, hi, K, voxel_size, batches, batch_size=10, seed=42):
    """SectionSource's augmented batches from one store (no mask dataset) without a device: the same stream, the same draw order
    (per slot: sample index, z, y, x until the summed-area test accepts, then draw_plan2d), the same per-slot rejection rounds,
    through the float64 map cast to float32.  Yields (raw centre channel over the output window (S, h, w), labels over the
    output window (S, h, w)) per batch."""
    from bootstrapper_amd import augment2d as A
    rng = np.random.default_rng(seed)
    h, w = out
    need = -(-5 * h * w // 100)
    ctx = [(i - o) // 2 for i, o in zip(inp, out)]
    frame = A.frame_of(inp, out, lo, hi)
    known = (labels > 0).astype(np.int64)
    sat = np.zeros((labels.shape[0], labels.shape[1] + 1, labels.shape[2] + 1), dtype=np.int64)
    sat[:, 1:, 1:] = known.cumsum(1).cumsum(2)
    win = sat[:, h:, w:] - sat[:, :-h, w:] - sat[:, h:, :-w] + sat[:, :-h, :-w]
    has = win.reshape(win.shape[0], -1).max(axis=1) >= need     # sections that hold an acceptable window keep their table

    def draw():
        while True:
            rng.integers(1)
            z, y, x = (int(rng.integers(0, s - o + 1)) for s, o in zip(labels.shape, (1, h, w)))
            if has[z] and win[z, y, x] >= need:
                return z, y, x
    lab64 = labels.astype(np.int64)
    for _ in range(batches):
        raw_b = np.zeros((batch_size, h, w))
        lab_b = np.zeros((batch_size, h, w), dtype=np.int64)
        slots = list(range(batch_size))
        while slots:
            failed = []
            for s in slots:
                z, y, x = draw()
                plan = A.draw_plan2d(rng, params, inp, frame, K, voxel_size)
                blo, bhi = A.source_box2d(plan)
                size = (bhi[0] - blo[0], bhi[1] - blo[1])
                start = (y - ctx[0] + blo[0], x - ctx[1] + blo[1])
                coords = map_f64(plan, blo).astype(np.float32)
                region = (tuple(ctx), (h, w))
                lab = sample_nearest(_window(coords[K // 2], plan, region), read_padded(lab64[z], start, size))
                if int((lab > 0).sum()) < need:
                    failed.append(s)
                    continue
                ks = K - 1 - K // 2 if plan.mirror[0] else K // 2
                zz = z - K // 2 + ks
                rsec = read_padded(raw[zz], start, size) if 0 <= zz < raw.shape[0] else np.zeros(size, dtype=raw.dtype)
                raw_b[s] = bilinear_f64(_window(coords[K // 2], plan, region), rsec) * 2.0 / 255.0 - 1.0
                lab_b[s] = lab
            slots = failed
        yield raw_b, lab_b
