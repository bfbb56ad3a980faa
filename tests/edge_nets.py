"""Case E of the per-launch suites: nets whose channel counts sit on the edges of the launchers' tile and padding rules.  Plain data
plus a builder, read by tests/test_layers_edges_gpu.py and tests/test_backward_edges_gpu.py.  No GPU needed to import it.

Every net has in_channels = 1, 3x3x3 kernels in every pass, (1, 2, 2) pooling and a 3d_affs head of 6 channels, as C_NET of
tests/test_layers_gpu.py has; level l holds a * k^l channels (a = num_fmaps, k = fmap_inc_factor), the decoder pass of level l reads
a k^l + a k^(l+1).  Level 0 stays at 64 channels or fewer: the head kernel takes no more.

  net  (a, k)    deepest level -> GEMM tile columns x N-tiles      what else it pins
  E1   (16, 4)   64  -> 64 x 1 exact      level 0 at 16 exact (first pass, box, halo-resident Npad 16); wgrad N = 64, C = 64; decoder cin 80
  E2   (11, 3)   33  -> 64 x 1            one over the 32-column tile; Cpad 48; wgrad N = 33, C = 33
  E3   (13, 5)   65  -> 160 x 1           one over 64; wgrad N = 65 (128-tile), C = 65 (a second C-tile with one real channel)
  E4   (32, 5)   160 -> 160 x 1 exact     level 0 at 32 exact; F(4x4) at Cpad 160; dgrad N = 192
  E5   (23, 7)   161 -> 256 x 1           a single 256-column tile, 95 padding columns; Cpad 176 (11 units) in the Winograd V
  E6   (64, 4)   256 -> 256 x 1 exact     level 0 at 64 exact (the head's limit); decoder 320 -> 64; dgrad N = 320 exact
  E7   (16, 19)  304 -> 320 x 1, CUT      exactly 16 padding columns: the Co <= 304 boundary from below
  E8   (61, 5)   305 -> 320 x 1, no CUT   the same boundary from above; decoder 366 -> 61
  E9   (64, 5)   320 -> 320 x 1 exact     decoder 384 -> 64; dgrad N = 384 -> 2 x 256, the last tile exactly half full
  E10  (40, 10)  400 -> 256 x 2           two N-tiles at a small shape; decoder 440 -> 40: below-up dense at Cpad 48
  E11  (32, 15)  480 -> 256 x 2           decoder 512 -> 32: below-up dense at Cpad 32, the F(4x4) rule's cout >= 32 edge
  E12  (16, 33)  528 -> 320 x 2           two 320-column tiles, no CUT
  E13  (40, 4), three levels 40 / 160 / 640: 640 -> 320 x 2 exact; the pooled output stored by the output transform of 160 -> 160;
                                          decoder 800 -> 160

E1 - E12 run at (13, 36, 40): the smallest input that passes two levels and gives every stage more than one 256-row GEMM tile with a
partial last one -- stage outputs (11, 34, 38) 14 212 rows, (9, 32, 36) 10 368, (7, 14, 16) 1 568, (5, 12, 14) 840, (3, 22, 26) 1 716,
(1, 20, 24) 480; the Winograd stages get overhanging 4 x 4 tiles in y (14, 22) and x (14, 26) and exact ones (16, 12, 20, 24).
E13 runs at (21, 48, 52): stage outputs (19, 46, 50), (17, 44, 48), (15, 20, 22), (13, 18, 20), (11, 7, 8) 616 rows, (9, 5, 6) 270 rows
-- the deepest stage has two row tiles, the second with 14 rows --, (7, 8, 10), (5, 6, 8) 240 rows and (1, 8, 12) 96 rows: the last two
are a single partial tile.
"""
import numpy as np

SHAPE = (13, 36, 40)
# tag -> (num_fmaps, fmap_inc_factor, levels, input shape)
NETS = {
    "E1": (16, 4, 2, SHAPE), "E2": (11, 3, 2, SHAPE), "E3": (13, 5, 2, SHAPE), "E4": (32, 5, 2, SHAPE), "E5": (23, 7, 2, SHAPE),
    "E6": (64, 4, 2, SHAPE), "E7": (16, 19, 2, SHAPE), "E8": (61, 5, 2, SHAPE), "E9": (64, 5, 2, SHAPE), "E10": (40, 10, 2, SHAPE),
    "E11": (32, 15, 2, SHAPE), "E12": (16, 33, 2, SHAPE), "E13": (40, 4, 3, (21, 48, 52)),
}
TAGS = list(NETS)
BACKWARD_TAGS = ["E1", "E3", "E4", "E6", "E9", "E10", "E13"]
VARIANT_TAGS = ["E1", "E5", "E6", "E13"]
# the rows of every stage of E1 - E12, in the planner's order (the docstring's list; test_edge_shapes_keep_their_properties holds it)
STAGE_ROWS = [14212, 10368, 1568, 840, 1716, 480]

_K3 = [[3, 3, 3], [3, 3, 3]]


def net_config(tag):
    a, k, levels, _ = NETS[tag]
    return {"in_channels": 1, "num_fmaps": a, "fmap_inc_factor": k, "downsample_factors": [[1, 2, 2]] * (levels - 1),
            "kernel_size_down": [_K3] * levels, "kernel_size_up": [_K3] * (levels - 1), "outputs": {"3d_affs": {"dims": 6}}}


def shape_of(tag):
    return NETS[tag][3]


def edge_case(tag, seed=3):
    """(net config, state dict, raw uint8 (D, H, W)): synthetic weights, seeded noise as raw"""
    from bootstrapper_amd.synth import synthetic_state_dict
    nc = net_config(tag)
    raw = np.random.default_rng(7).integers(0, 256, size=shape_of(tag), dtype=np.uint8)
    return nc, synthetic_state_dict(nc, seed), raw
