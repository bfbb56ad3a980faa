"""ctypes binding of libbsmi.so (include/bsmi.h).  There is no fallback: if the
library is missing or a symbol is absent, importing this module raises."""
import ctypes as C
import os

# PyTorch first: it brings its own copy of the HIP runtime (same soname as /opt/rocm's), and the process must bind
# ONE of them.  Loading libbsmi.so before torch starts a second runtime, whose calls then fail with
# "no ROCm-capable device is detected" while torch's work.
import torch  # noqa: F401,E402

_HERE = os.path.dirname(os.path.abspath(__file__))
# BSMI_LIB: developer knob to A/B another build of the same library (never a fallback)
LIB_PATH = os.environ.get("BSMI_LIB") or os.path.join(_HERE, "libbsmi.so")

MAX_LEVELS, MAX_CONVS, MAX_HEADS, NAME_LEN = 8, 4, 4, 32
PREC_F32, PREC_BF16, PREC_BF16X3 = 0, 1, 2
RAW_U8, RAW_F32, RAW_U8_UNIT = 0, 1, 2
ERR_INVALID, ERR_HIP, ERR_STATE, ERR_MISSING, ERR_OVERFLOW = -1, -2, -3, -4, -5


class UNetConfig(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32),
        ("num_fmaps", C.c_int32),
        ("fmap_inc_factor", C.c_int32),
        ("num_levels", C.c_int32),
        ("downsample_factors", (C.c_int32 * 3) * MAX_LEVELS),
        ("n_convs_down", C.c_int32 * MAX_LEVELS),
        ("kernel_size_down", ((C.c_int32 * 3) * MAX_CONVS) * MAX_LEVELS),
        ("n_convs_up", C.c_int32 * MAX_LEVELS),
        ("kernel_size_up", ((C.c_int32 * 3) * MAX_CONVS) * MAX_LEVELS),
        ("num_heads", C.c_int32),
        ("head_name", (C.c_char * NAME_LEN) * MAX_HEADS),
        ("head_dims", C.c_int32 * MAX_HEADS),
        ("num_fmaps_out", C.c_int32),
    ]


class StepInfo(C.Structure):
    """bsmi_unet_step_info of include/bsmi.h"""
    _fields_ = [("type", C.c_int32), ("materialised", C.c_int32), ("shape", C.c_int32 * 4), ("conv_index", C.c_int32),
                ("form", C.c_int32), ("flags", C.c_int32), ("bn", C.c_int32), ("ksteps", C.c_int32), ("head", C.c_int32),
                ("factor", C.c_int32 * 3), ("offset", C.c_int32 * 3), ("prefix", C.c_char * 64)]


class TrainWgradInfo(C.Structure):
    """bsmi_unet_train_wgrad_info of include/bsmi.h"""
    _fields_ = [(n, C.c_int32) for n in ("family", "residual", "n", "c", "cbase", "kx", "tile_n", "tile_c", "ranges", "lines_per_range",
                                         "det_workspace")]


class TrainStepInfo(C.Structure):
    """bsmi_unet_train_step_info of include/bsmi.h"""
    _fields_ = [("type", C.c_int32), ("n_wgrad", C.c_int32), ("wgrad", TrainWgradInfo * 4), ("dgrad", C.c_int32), ("dgrad_raw", C.c_int32),
                ("dgrad_converted", C.c_int32), ("dgrad_bn", C.c_int32), ("dgrad_ksteps", C.c_int32), ("dgrad_split_k", C.c_int32),
                ("dgrad_scatter", C.c_int32), ("dgrad_residual", C.c_int32), ("border", C.c_int32 * 3), ("has_split", C.c_int32),
                ("bias", C.c_int32), ("up", C.c_int32), ("fwd_split", C.c_int32), ("deterministic", C.c_int32)]


WGRAD_FAMILIES = ("none", "wave-f32", "tiled-f32", "split-bf16")
TRAIN_TENSORS = {"dout": 0, "gmask": 1, "gsplit": 2, "gsplit_hi": 3, "gsplit_lo": 4, "dcat": 5, "head_dp": 6, "pad_count": 7}
STEP_TYPES = ("input", "conv", "pool", "up", "head")
CONV_FORMS = ("gather", "raster-halo", "box-halo", "halo-resident", "first-pass", "winograd F(2x2)", "winograd F(4x4)")
STEP_FLAGS = {1: "fused-up", 2: "res-low", 4: "split-k"}
STEP_BELOW_UP = 8  # reported as plan_steps()'s own key `below_up`, not among the flags
STEP_WINO_Z = 16   # ... and `wino_z`: the F(4x4) stage is F(2,3) along z as well (csrc/unet_rules.hip wino_z_site)


class Codec(C.Structure):
    """bsmi_codec of include/bsmi_io.h"""
    _fields_ = [("id", C.c_int32), ("level", C.c_int32), ("cname", C.c_int32), ("shuffle", C.c_int32),
                ("typesize", C.c_int32), ("blocksize", C.c_int32)]


class ChunkCopy(C.Structure):
    """bsmi_chunk_copy of include/bsmi_io.h"""
    _fields_ = [("path", C.c_char_p), ("base", C.c_void_p), ("start", C.c_int64 * 4), ("extent", C.c_int64 * 4),
                ("stride", C.c_int64 * 4), ("read_modify_write", C.c_int32), ("reserved", C.c_int32)]


class BatchFragArgs(C.Structure):
    """bsmi_batch_frag_args of include/bsmi.h"""
    _fields_ = [("affs_dev", C.c_void_p), ("frags_dev", C.c_void_p), ("max_id_dev", C.c_void_p), ("labels_dev", C.c_void_p),
                ("num_labels_dev", C.c_void_p), ("id_offset", C.c_uint64), ("size_dev", C.c_void_p), ("sums_dev", C.c_void_p)]


class BatchGraphArgs(C.Structure):
    """bsmi_batch_graph_args of include/bsmi.h"""
    _fields_ = [("affs_dev", C.c_void_p), ("frags_dev", C.c_void_p), ("edges_dev", C.c_void_p), ("sums_dev", C.c_void_p),
                ("pair_counts_dev", C.c_void_p), ("counts_dev", C.c_void_p), ("edge_capacity", C.c_uint64)]


class Aug2dDraw(C.Structure):
    """bsmi_aug2d_draw of include/bsmi.h (64 bytes)"""
    _fields_ = [("a", C.c_float * 4), ("src", C.c_float * 2), ("inv_spacing", C.c_float * 2), ("flags", C.c_int32), ("n", C.c_int32 * 2),
                ("lattice_offset", C.c_int32), ("crop", C.c_int32 * 2), ("crop_offset", C.c_int32), ("reserved", C.c_int32)]


class Aug2dIDraw(C.Structure):
    """bsmi_aug2d_idraw of include/bsmi.h (48 bytes)"""
    _fields_ = [("seed", C.c_uint64), ("impulse_threshold", C.c_uint64), ("noise_sigma", C.c_float), ("contrast_scale", C.c_float),
                ("nodes", C.c_int32), ("radius", C.c_int32), ("taps_offset", C.c_int32), ("reserved", C.c_int32 * 3)]


CODEC_RAW, CODEC_ZLIB, CODEC_GZIP, CODEC_ZSTD, CODEC_LZ4, CODEC_BLOSC = range(6)
BLOSC_LZ4, BLOSC_ZLIB, BLOSC_ZSTD = 1, 3, 4
CHUNK_MISSING = 1
MORPH_DILATE, MORPH_ERODE = 0, 1
RESCALE_DOWN, RESCALE_UP = 0, 1


class BsmiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libbsmi error {code}: {msg}")
        self.code = code
        self.msg = msg


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C bootstrapper_amd/csrc`).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    p, i32, i64p, vp = C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_void_p
    sigs = {
        "bsmi_last_error": (C.c_char_p, []),
        "bsmi_version": (i32, []),
        "bsmi_unet_create": (i32, [C.POINTER(UNetConfig), i32, C.POINTER(p)]),
        "bsmi_unet_destroy": (i32, [p]),
        "bsmi_unet_load_weight": (i32, [p, C.c_char_p, vp, i64p, i32]),
        "bsmi_unet_finalize": (i32, [p, i32]),
        "bsmi_unet_output_shape": (i32, [p, i64p, i64p]),
        "bsmi_unet_flops": (i32, [p, i64p, C.POINTER(C.c_double)]),
        "bsmi_unet_forward": (i32, [p, i32, vp, i32, i64p, C.POINTER(vp), C.POINTER(vp), vp]),
        "bsmi_unet_debug_activation": (i32, [p, i32, i32, i64p, vp, C.c_uint64]),
        "bsmi_unet_debug_step_info": (i32, [p, i32, C.POINTER(StepInfo), C.POINTER(i32)]),
        "bsmi_debug_wino_pack_host": (i32, [vp, i32, i32, i32, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                            C.POINTER(i32), C.POINTER(i32)]),
        "bsmi_unet_profile_enable": (i32, [p, i32]),
        "bsmi_unet_profile_read": (i32, [p, i32, C.POINTER(i32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                         C.POINTER(C.c_double)]),
        "bsmi_unet_profile_totals": (i32, [p, C.POINTER(C.c_double), C.POINTER(C.c_double), i64p, i32]),
        "bsmi_extract_block_reflect_u8": (i32, [vp, i64p, i64p, i64p, vp, vp]),
        "bsmi_seg_create": (i32, [i32, i64p, C.POINTER(p)]),
        "bsmi_seg_destroy": (i32, [p]),
        "bsmi_ws_fragments_u8": (i32, [p, vp, i64p, i32, i32, vp, vp, vp]),
        "bsmi_ws_fragments_seeds_u8": (i32, [p, vp, i64p, i32, i32, vp, vp, vp, vp]),
        "bsmi_rag_agglomerate_u8": (i32, [p, vp, vp, i64p, C.c_float, C.c_int, vp]),
        "bsmi_rag_edge_stats": (i32, [p, vp, vp, C.c_uint64, vp]),
        "bsmi_agglomerate_mean_u8": (i32, [p, vp, vp, i64p, C.POINTER(C.c_float), i32, vp, vp]),
        "bsmi_agglomerate_hist_u8": (i32, [p, vp, vp, i64p, C.POINTER(C.c_float), i32, i32, i32, vp, vp]),
        "bsmi_agglomerate_hist_graph": (i32, [C.c_uint32, C.c_uint32, vp, vp, vp, i32, i32, C.POINTER(C.c_float), i32, vp]),
        "bsmi_frag_postprocess_u8": (i32, [p, vp, vp, i64p, C.c_double, C.c_int64, i64p, i64p, C.c_uint64, vp, vp, vp]),
        "bsmi_label_stats": (i32, [p, vp, i64p, C.c_uint64, C.c_uint64, vp, vp, vp]),
        "bsmi_rag_merge_scores_u8": (i32, [p, vp, vp, i64p, C.c_float, C.c_int, vp, vp, C.c_uint64, vp, vp, vp, vp]),
        "bsmi_lut_relabel": (i32, [C.c_int, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp]),
        "bsmi_lut_relabel_multi": (i32, [i32, vp, C.c_uint64, vp, vp, C.c_uint64, i32, vp, vp]),
        "bsmi_connected_components": (i32, [vp, C.c_uint64, vp, vp, C.c_uint64, C.c_float, vp]),
        "bsmi_connected_components_multi": (i32, [vp, C.c_uint64, vp, vp, C.c_uint64, vp, C.c_int, vp]),
        "bsmi_cc_affs_u8": (i32, [p, vp, i64p, C.c_int, C.c_int64, vp, vp, vp, vp]),
        "bsmi_mws_agglom_f64": (i32, [C.c_int, vp, C.c_int, vp, vp, C.c_uint32, i64p, vp, vp]),
        "bsmi_mws_cluster": (i32, [C.c_uint64, vp, vp, C.c_uint64, vp]),
        "bsmi_frag_pair_affinity_u8": (i32, [C.c_int, vp, C.c_int, vp, vp, i64p, C.c_uint64, vp, vp, vp, vp, vp]),
        "bsmi_label_table_u64": (i32, [p, vp, i64p, C.c_int64, vp, vp, vp, vp, C.c_uint64, vp, vp]),
        "bsmi_seg_status": (i32, [p, vp]),
        "bsmi_seg_set_host_flood": (i32, [p, i32]),
        "bsmi_seg_batch_create": (i32, [C.POINTER(p), i32, C.POINTER(p)]),
        "bsmi_seg_batch_destroy": (i32, [p]),
        "bsmi_seg_batch_fragments_u8": (i32, [p, i32, C.POINTER(BatchFragArgs), i64p, i32, i32, C.c_double, C.c_int64, i64p, i64p, C.c_uint64, vp]),
        "bsmi_seg_batch_rag_graph_u8": (i32, [p, i32, C.POINTER(BatchGraphArgs), i64p, vp]),
        "bsmi_rag_graph_u8": (i32, [p, vp, vp, i64p, vp, vp, vp, C.c_uint64, vp, vp]),
        "bsmi_rag_merge_scores_host": (i32, [i32, vp, vp, vp, vp, C.c_float, i32, vp, i32]),
        "bsmi_rag_merge_scores_host_rule": (i32, [i32, vp, vp, vp, vp, C.c_float, i32, i32, vp, i32]),
        "bsmi_unet_train_set_arithmetic": (i32, [p, i32]),
        "bsmi_unet_train_set_deterministic": (i32, [p, i32]),
        "bsmi_unet_train_begin": (i32, [p, i64p]),
        "bsmi_unet_train_forward_backward": (i32, [p, vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_float), vp]),
        "bsmi_unet_train_num_params": (i32, [p, C.POINTER(C.c_uint64)]),
        "bsmi_unet_train_buffers": (i32, [p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
        "bsmi_unet_train_param_info": (i32, [p, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "bsmi_unet_train_adam_step": (i32, [p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, vp]),
        "bsmi_unet_train_read_param": (i32, [p, C.c_char_p, C.c_int, vp]),
        "bsmi_unet_train_last_loss": (i32, [p, C.POINTER(C.c_float), vp]),
        "bsmi_unet_train_prediction": (i32, [p, i32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
        "bsmi_unet_train_grad_groups": (i32, [p, i32, C.POINTER(i32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "bsmi_unet_train_wait_grad_group": (i32, [p, i32, vp]),
        "bsmi_unet_train_write_param": (i32, [p, C.c_char_p, C.c_int, vp]),
        "bsmi_unet_train_step_count": (i32, [p, C.c_int, C.POINTER(C.c_int)]),
        "bsmi_unet_train_end": (i32, [p]),
        "bsmi_unet_train_debug_tensor": (i32, [p, i32, i32, i64p, vp, C.c_uint64]),
        "bsmi_unet_train_debug_step_info": (i32, [p, i32, C.POINTER(TrainStepInfo)]),
        "bsmi_train_affinity_targets": (i32, [C.c_int, vp, vp, i64p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_float,
                                              C.c_float, vp, vp, vp]),
        "bsmi_train_lsd_targets": (i32, [C.c_int, vp, vp, i64p, i64p, i64p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, vp, vp, vp]),
        "bsmi_train_lsd2d_targets": (i32, [C.c_int, vp, vp, C.c_int, i64p, i64p, i64p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int,
                                           vp, vp, vp]),
        "bsmi_train_affinity_targets_roi": (i32, [C.c_int, vp, vp, C.c_int, i64p, i64p, i64p, C.POINTER(C.c_int32), C.c_int, C.c_int,
                                                  C.c_int, C.c_float, C.c_float, vp, vp, vp]),
        "bsmi_train_mask_sat": (i32, [C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
        "bsmi_unet_set_persistent_grid": (i32, [p, C.c_int]),
        "bsmi_unet_profile_executed": (i32, [p, C.POINTER(C.c_double), C.c_int]),
        "bsmi_debug_lds_canary": (i32, [i32, i32, i32, vp, vp]),
        "bsmi_debug_check_guards": (i32, []),
        "bsmi_debug_torch_malloc": (vp, [C.c_ssize_t, i32, vp]),
        "bsmi_debug_torch_free": (None, [vp, C.c_ssize_t, vp]),
        "bsmi_debug_guard_selftest": (i32, []),
        "bsmi_stream_create_cu_mask": (i32, [C.c_int, vp, C.c_int, C.POINTER(C.c_void_p)]),
        "bsmi_stream_destroy": (i32, [C.c_int, vp]),
        "bsmi_eval_create": (i32, [i32, C.c_uint64, C.POINTER(p)]),
        "bsmi_eval_destroy": (i32, [p]),
        "bsmi_eval_aff_errors_u8": (i32, [p, vp, i64p, i64p, vp, i32, i64p, vp, C.POINTER(C.c_int32), i64p, C.c_float, C.c_float,
                                          C.c_int64, vp, vp, vp, vp]),
        "bsmi_eval_lsd_errors_u8": (i32, [p, vp, i64p, i64p, vp, vp, i64p, i64p, i64p, i64p, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                          i32, C.c_float, C.c_float, C.c_int64, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp]),
        "bsmi_eval_pairs_u64": (i32, [p, vp, vp, vp, i64p, i32, vp]),
        "bsmi_eval_pairs_read": (i32, [p, vp, vp, vp, C.c_uint64, vp, vp]),
        "bsmi_eval_status": (i32, [p, vp]),
        "bsmi_label_morph_u64": (i32, [i32, vp, i64p, i32, i32, i32, vp, vp, vp]),
        "bsmi_label_fill_holes_scratch_bytes": (C.c_size_t, [i64p, C.c_uint64]),
        "bsmi_label_fill_holes_u64": (i32, [i32, vp, i64p, i32, vp, vp, C.c_size_t, C.c_uint64, C.POINTER(C.c_uint64), vp]),
        "bsmi_mask_closing_work_bytes": (C.c_size_t, [i64p, i32]),
        "bsmi_mask_closing_disk_u8": (i32, [i32, vp, i64p, i32, vp, vp, C.c_size_t, vp]),
        "bsmi_downscale_mean": (i32, [i32, vp, i32, i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, i64p, vp]),
        "bsmi_rescale_sample": (i32, [i32, vp, i32, i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), i32, vp, i64p, vp]),
        "bsmi_nonzero_bbox": (i32, [i32, vp, i32, i64p, i64p, vp, vp]),
        "bsmi_synth_create": (i32, [i32, i64p, C.POINTER(p)]),
        "bsmi_synth_destroy": (i32, [p]),
        "bsmi_synth_dilate_points": (i32, [p, i64p, vp, i32, vp, vp, vp, vp, vp]),
        "bsmi_synth_label_i32": (i32, [p, vp, i64p, vp, C.POINTER(C.c_uint64), vp]),
        "bsmi_synth_expand_i32": (i32, [p, vp, i64p, i32, C.c_int32, vp, vp]),
        "bsmi_synth_tubes_i32": (i32, [p, vp, i64p, vp, C.POINTER(C.c_uint64), vp]),
        "bsmi_synth_gaussian_f32": (i32, [p, vp, i64p, vp, i32, vp, vp]),
        "bsmi_synth_argmax_filter_f32": (i32, [p, vp, i64p, i32, vp, vp]),
        "bsmi_synth_basins_f32": (i32, [p, vp, vp, vp, i64p, vp, C.POINTER(C.c_uint64), vp]),
        "bsmi_synth_finish_i32": (i32, [p, vp, i64p, i32, i32, i32, vp, vp]),
        "bsmi_synth_grow_boundary_i64": (i32, [i32, vp, i64p, C.c_uint64, i32, vp, vp]),
        "bsmi_synth_merge_i64": (i32, [i32, vp, i64p, C.POINTER(C.c_int32), i32, C.c_int64, C.c_int64, vp]),
        "bsmi_synth_stamp_i64": (i32, [i32, vp, i64p, i32, i32, i32, vp, i32, i32, C.c_int64, vp]),
        "bsmi_synth_present_i64": (i32, [p, vp, C.c_uint64, vp, C.c_uint32, C.POINTER(C.c_uint32), vp]),
        "bsmi_synth_split_i64": (i32, [p, vp, i64p, C.c_int64, i32, C.POINTER(C.c_int32), i32, C.c_int64, C.POINTER(C.c_uint64), vp]),
        "bsmi_aug_coords": (i32, [i32, i64p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), i32, i32, vp, vp,
                                  C.POINTER(C.c_int32), C.POINTER(C.c_float), vp, vp]),
        "bsmi_aug_sample_f32_u8": (i32, [i32, vp, i64p, i64p, i64p, vp, i64p, vp, vp]),
        "bsmi_aug_sample_nearest_i64": (i32, [i32, vp, i64p, i64p, i64p, vp, i64p, vp, vp]),
        "bsmi_aug_sample_nearest_u8": (i32, [i32, vp, i64p, i64p, i64p, vp, i64p, vp, vp]),
        "bsmi_aug_sample_unit_f32_u8": (i32, [i32, vp, i64p, i64p, i64p, vp, i64p, vp, vp]),
        "bsmi_aug_noise_f32": (i32, [i32, i64p, vp, C.c_uint64, C.c_float, vp]),
        "bsmi_aug_section_stats_f32": (i32, [i32, i64p, vp, vp, vp, vp]),
        "bsmi_aug_intensity_f32": (i32, [i32, i64p, vp, vp, vp, vp, vp]),
        "bsmi_aug_gamma_f32": (i32, [i32, i64p, vp, vp, vp, vp]),
        "bsmi_aug_impulse_f32": (i32, [i32, i64p, vp, C.c_uint64, C.c_uint64, vp]),
        "bsmi_aug_smooth_f32": (i32, [i32, i64p, vp, vp, C.POINTER(C.c_float), i32, vp]),
        "bsmi_aug_defect_f32": (i32, [i32, i64p, vp, vp, vp, C.c_float, i32, vp]),
        "bsmi_aug2d_coords": (i32, [i32, C.POINTER(Aug2dDraw), vp, i32, i32, i64p, i64p, i64p, vp, vp, C.c_int64, vp, vp]),
        "bsmi_aug2d_sample_f32_u8": (i32, [i32, C.POINTER(Aug2dDraw), vp, i32, i32, vp, i64p, i64p, i64p, vp, C.c_int64, vp, vp]),
        "bsmi_aug2d_sample_nearest_i64": (i32, [i32, C.POINTER(Aug2dDraw), vp, i32, i32, vp, i64p, i64p, i64p, vp, C.c_int64, vp, vp]),
        "bsmi_aug2d_sample_nearest_u8": (i32, [i32, C.POINTER(Aug2dDraw), vp, i32, i32, vp, i64p, i64p, i64p, vp, C.c_int64, vp, vp]),
        "bsmi_aug2d_sample_unit_f32_u8": (i32, [i32, C.POINTER(Aug2dDraw), vp, C.POINTER(Aug2dIDraw), vp, i32, i32, vp, i64p, i64p, i64p, vp,
                                                C.c_int64, vp, vp]),
        "bsmi_aug2d_noise_f32": (i32, [i32, C.POINTER(Aug2dIDraw), vp, i32, i32, i64p, vp, vp]),
        "bsmi_aug2d_intensity_f32": (i32, [i32, C.POINTER(Aug2dIDraw), vp, i32, i32, i64p, vp, vp, vp, vp, vp]),
        "bsmi_aug2d_gamma_f32": (i32, [i32, C.POINTER(Aug2dIDraw), vp, i32, i32, i64p, vp, vp, vp, vp]),
        "bsmi_aug2d_impulse_f32": (i32, [i32, C.POINTER(Aug2dIDraw), vp, i32, i32, i64p, vp, vp]),
        "bsmi_aug2d_smooth_f32": (i32, [i32, C.POINTER(Aug2dIDraw), vp, i32, i32, i64p, vp, vp, vp, C.c_int64, vp]),
        "bsmi_aug2d_defect_f32": (i32, [i32, C.POINTER(Aug2dIDraw), vp, i32, i32, i64p, vp, vp, C.POINTER(C.c_int32), vp, i32, vp]),
        "bsmi_augin_group_mean_f32": (i32, [i32, i64p, vp, vp, i32, vp, vp]),
        "bsmi_augin_intensity_f32": (i32, [i32, i64p, vp, vp, vp, vp, i32, vp]),
        "bsmi_augin_smooth_f32": (i32, [i32, i64p, vp, vp, vp, vp, i32, vp]),
        "bsmi_augin_contrast_f32": (i32, [i32, i64p, vp, vp, vp, C.c_float, vp]),
        # include/bsmi_io.h
        "bsmi_codec_bound": (C.c_size_t, [C.POINTER(Codec), C.c_size_t]),
        "bsmi_codec_decode": (i32, [C.POINTER(Codec), vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        "bsmi_codec_encode": (i32, [C.POINTER(Codec), vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        "bsmi_chunks_read": (i32, [C.POINTER(Codec), i32, C.POINTER(C.c_char_p), C.POINTER(vp), C.POINTER(C.c_size_t),
                                   C.POINTER(C.c_size_t), C.POINTER(i32), i32]),
        "bsmi_chunks_write": (i32, [C.POINTER(Codec), i32, C.POINTER(C.c_char_p), C.POINTER(vp), C.POINTER(C.c_size_t),
                                    C.POINTER(i32), i32]),
        "bsmi_blosc_dev_frame_bound": (C.c_size_t, [C.c_size_t]),
        "bsmi_blosc_dev_scratch_bytes": (C.c_size_t, [i32, C.c_size_t]),
        "bsmi_blosc_encode_dev_u64": (i32, [i32, vp, C.c_int64, C.c_int64, i32, i64p, i64p, i64p, vp, C.c_size_t, vp, C.c_size_t, vp, vp]),
        "bsmi_blosc_dev_u8_frame_bound": (C.c_size_t, [C.c_size_t]),
        "bsmi_blosc_dev_u8_scratch_bytes": (C.c_size_t, [i32, C.c_size_t]),
        "bsmi_blosc_encode_dev_u8": (i32, [i32, vp, i64p, i32, i64p, i64p, i64p, vp, C.c_size_t, vp, C.c_size_t, vp, vp]),
        "bsmi_rag_write_sqlite": (i32, [C.c_char_p, C.c_uint64, vp, vp, vp, C.c_uint64, vp, vp]),
        "bsmi_chunks_read_into": (i32, [C.POINTER(Codec), i32, C.POINTER(ChunkCopy), i64p, i32, vp, C.POINTER(i32), i32]),
        "bsmi_chunks_write_from": (i32, [C.POINTER(Codec), i32, C.POINTER(ChunkCopy), i64p, i32, vp, C.POINTER(i32), i32]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    return lib, sorted(sigs)


lib, SYMBOLS = _load()


def check(rc):
    if rc != 0:
        raise BsmiError(rc, lib.bsmi_last_error().decode(errors="replace"))


def i64x3(v):
    return (C.c_int64 * 3)(*[int(x) for x in v])


def i64x4(v):
    return (C.c_int64 * 4)(*[int(x) for x in v])
