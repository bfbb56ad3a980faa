"""What tests/test_redzones_gpu.py runs between red zones, and what it leaves out.  Plain data, read by the GPU test, by its worker
and by tests/test_redzone_cases_cpu.py (which holds the three tables to the test files, to bootstrapper_amd/_lib.py and to
include/bsmi.h).

FAMILIES   family -> pytest node ids of GPU parity tests of the suite.  The worker runs the families one after the other in a process
           in which every torch tensor is allocated at its exact size between two guard zones (csrc/dev_guard.hip), and checks the
           zones after each, so the families are cut by engine: one damaged zone names few kernels.
WHOLE      files of which every test function runs between red zones (parameter sets may be thinned, see below).
EXCLUDED   entry point of the signature table of bootstrapper_amd/_lib.py -> why no family has to call it.  Host-only functions, and
           functions whose device memory is all their own engine's (guarded by BSMI_GUARD_MB itself, tests/guard_worker.py).  One with
           a `*_dev` parameter may stand here only with a reason that begins `needs:` and names what it needs.
NOT_USED   tests/test_*_gpu.py files that no family uses -> why.

A test is left out of a family only if it reaches torch.cuda.memory_reserved / memory_allocated (the pluggable allocator raises
there: utils._free_bytes, refine.morph, volume.SlabSegmenter, post/watershed.py), starts processes of its own (they would not have
the allocator) or uses more than one rank.

Time: the guard run is held to what tests/test_guards_gpu.py costs.  Where a family was over its share its largest parameter sets
were dropped, never the last node that reaches an entry point or a code path of its own (a regime of a sort, a kernel form, a branch of a
chain); what was dropped is said at the family.
Those cases still run in the plain suite."""

_SEG = "tests/test_seg_gpu.py::"
_SEGB = "tests/test_seg_batch_gpu.py::"
_MWS = "tests/test_mws_gpu.py::"
_MWSS = "tests/test_mws_scale_gpu.py::"
_EV = "tests/test_evaluate_gpu.py::"
_EVL = "tests/test_evaluate_lsd_gpu.py::"
_MO = "tests/test_morph_gpu.py::"
_UT = "tests/test_utils_gpu.py::"
_SY = "tests/test_synth_gpu.py::"
_TG = "tests/test_targets_gpu.py::"
_T2 = "tests/test_train2d_gpu.py::"
_TR = "tests/test_train_gpu.py::"
_UN = "tests/test_unet_gpu.py::"
_B8 = "tests/test_blosc_u8_gpu.py::"
_B64 = "tests/test_blosc_dev_gpu.py::"

FAMILIES = {
    # all but test_three_array_flood_in_subprocess (a child process).  Dropped for time, each a larger copy of a path that a kept case
    # takes: fragments at (16, 128, 128); agglomeration at (32, 128, 128); rag_agglomerate at (12, 64, 64); the post-processing at
    # (12, 96, 96) (crop, filter and size limit each stay in a smaller case); merge scores at (8, 96, 96) with 256 bins and small ids
    # (the later block's ids keep 256 bins); host scores at (12, 96, 96), (4, 160, 160) and the third tie case (6, 96, 96)
    "seg": [_SEG + n for n in (
        "test_fragments_bit_exact_vs_reference_goldens", "test_fragments_3d_mode_bit_exact", "test_fragments_bit_exact_vs_oracle[shape1-sigma1-10]",
        "test_fragments_bit_exact_vs_oracle[shape2-sigma2-7]", "test_fragments_bit_exact_vs_oracle[shape3-sigma3-10]",
        "test_fragments_of_odd_slices_bit_exact_vs_oracle", "test_fragments_white_noise_heap_spill",
        "test_ws_fragments_without_seeds_entry_equals_the_wrapper_s",
        "test_agglomeration_bit_exact_vs_oracle[shape0-sigma0]", "test_agglomeration_bit_exact_vs_oracle[shape2-sigma2]",
        "test_rag_agglomerate_in_place_equals_the_oracle[shape0-sigma0-0.3]", "test_label_table_equals_numpy",
        "test_agglomeration_edge_cases", "test_mirror_api_generator",
        "test_fragment_postprocess_bit_exact_vs_oracle[shape1-crop1-0.45-0]", "test_fragment_postprocess_bit_exact_vs_oracle[shape2-crop2-0.0-30]",
        "test_fragment_postprocess_bit_exact_vs_oracle[shape3-crop3-0.0-0]", "test_fragment_postprocess_serpentine_components",
        "test_rag_merge_scores_bit_exact_vs_oracle[shape1-sigma1-4-256-6291456]",
        "test_rag_merge_scores_bit_exact_vs_oracle[shape2-sigma2-6-16-1099511627781]", "test_rag_merge_scores_bit_exact_vs_oracle[shape3-sigma3-3-1-0]",
        "test_rag_scores_on_the_host_equal_the_device_loop_and_the_oracle[shape2-sigma2-5-256-0.45-0]",
        "test_rag_scores_on_the_host_equal_the_device_loop_and_the_oracle[shape3-sigma3-3-16-1.0-0]",
        "test_rag_scores_on_the_host_equal_the_device_loop_and_the_oracle[shape4-sigma4-3-256-1.0-3]",
        "test_rag_scores_on_the_host_equal_the_device_loop_and_the_oracle[shape5-sigma5-3-16-1.0-2]",
        "test_rag_merge_scores_threshold_leaves_unmerged_edges", "test_lut_relabel", "test_lut_relabel_multi_equals_single_columns",
        "test_cc_affs_bit_exact_vs_reference_goldens_and_oracle", "test_merge_rule_hand_built_graphs",
        "test_tie_rich_agglomeration_bit_exact_vs_oracle", "test_overflow_of_an_earlier_call_is_remembered")],
    # all but the two test_pipeline_* (VolumePipeline asks torch for allocator statistics)
    "seg_batch": [_SEGB + n for n in (
        "test_fragments_and_graph_equal_the_single_block_calls", "test_one_block_in_a_batch_of_five_workspaces",
        "test_an_overflow_marks_its_own_workspace_only", "test_slices_off_the_lds_path_are_refused")],
    # test_mws_gpu.py without its driver test; of the sort regimes of test_mws_scale_gpu.py the smallest case of each (one block: 1,024
    # candidates with chains and with cycles; merge sort: 1,025, the same two; onesweep: 1,052,672, no smaller one reaches it)
    "mws": [_MWS + n for n in (
        "test_grid_mutex_watershed_matches_restatement", "test_ties_zero_and_nan_edges", "test_graph_mutex_watershed_and_pair_affinities",
        "test_mwatershed_from_affinities_mirror")] + [_MWSS + n for n in (
        "test_sort_regimes[1x32x32-K1]", "test_sort_regimes[1x16x16-K4]", "test_sort_regimes[1x25x41-K1]", "test_sort_regimes[1x5x41-K5]",
        "test_sort_regimes[4x256x257-K4]", "test_mixed_sign_offsets", "test_pair_affinities_mixed_sign_offsets",
        "test_special_values_on_the_device", "test_constraints_inherited_over_a_long_sweep", "test_randomized_strides",
        "test_pair_affinities_at_scale", "test_pair_affinity_sum_beyond_24_bits", "test_pair_affinities_grow_their_capacity")],
    # all but test_evaluate_end_to_end (run_segmentation).  Dropped for time: of the affinity errors the two mixed mask / neighbourhood
    # cases; of the LSD errors, whose whole chain runs at every configuration, the repeats of a configuration in the per-stage tests
    # (the descriptors keep the anisotropic and one down-sampled case, the later stages the down-sampled one and margin 0, which only
    # they have)
    "eval": [_EV + n for n in (
        "test_errors_bit_equal_to_restatement[mask-negative]", "test_errors_bit_equal_to_restatement[nomask-positive]",
        "test_errors_at_the_dataset_edge_and_an_all_zero_chunk", "test_errors_other_channel_counts",
        "test_contingency_counts_equal_unique", "test_undersized_table_reports_overflow", "test_metrics_match_restatement")] + [_EVL + n for n in (
        "test_descriptors_against_the_oracle[aniso]", "test_descriptors_against_the_oracle[iso-df2]",
        "test_later_stages_bit_equal_on_the_device_s_own_outputs[iso-df2]", "test_later_stages_bit_equal_on_the_device_s_own_outputs[margin0]",
        "test_whole_chain_against_the_restatement", "test_chunk_groups_give_the_same_outputs", "test_driver_on_a_store")],
    # the stencil and fill-holes tests; the others go through refine.morph, which asks for allocator statistics
    "morph": [_MO + n for n in (
        "test_stencil_ops_bit_equal_to_restatement", "test_invalid_arguments_are_refused", "test_fill_holes_hand_made_cases",
        "test_fill_holes_bit_equal_to_restatement", "test_fill_holes_table_overflow_is_reported_and_the_wrapper_grows_the_table")],
    # the four kernel tests and their refusals; the others go through utils._free_bytes
    "utils": [_UT + n for n in (
        "test_closing_bit_equal_to_restatement", "test_closing_refuses_bad_arguments", "test_downscale_mean_bit_equal_to_restatement",
        "test_rescale_sample_bit_equal_to_restatement", "test_scale_kernels_refuse_bad_arguments", "test_nonzero_bbox",
        "test_bbox_refuses_bad_arguments")],
    # of the 24 dilations (3 shapes x 4 structures x 1 or 10 iterations): every shape, every structure, both counts
    "synth": [_SY + n for n in (
        "test_dilation[10-star-shape0]", "test_dilation[10-star-shape1]", "test_dilation[10-star-shape2]", "test_dilation[10-disk-shape1]",
        "test_dilation[10-ellipse-shape1]", "test_dilation[10-cross-shape2]", "test_dilation[1-cross-shape0]", "test_dilation[1-disk-shape2]",
        "test_dilation_per_section_tables_and_refusal", "test_tubes_branch", "test_expand_tie_rule",
        "test_gaussian_against_float64", "test_argmax_filter_and_basins", "test_random_branch", "test_argmax_filter_even_window_and_mask",
        "test_finish", "test_grow_boundary", "test_merge_stamp_present", "test_split", "test_obfuscate_follows_the_operation_list")],
    # of the intensity and input chains, whose case "all" runs every node of the chain: "all" at every block, and the variants that
    # change a launch (smooth05: radius 2; smooth_plane: no smoothing across channels) at the odd-sized blocks; the single-node cases
    # are the same launches once more
    "aug": ["tests/test_aug_gpu.py::" + n for n in (
        "test_launches_vs_reference", "test_identity_plan_returns_the_centre_crop", "test_mirror_only_plans_are_flips",
        "test_swap_only_plan_is_a_transpose", "test_integer_shift_only_plan_shifts_each_section", "test_odd_block_without_swap",
        "test_refusals")] + ["tests/test_intensity_gpu.py::" + n for n in (
        "test_launches_vs_reference[5x24x24-all]", "test_launches_vs_reference[3x17x33-all]", "test_launches_vs_reference[1x20x20-all]",
        "test_launches_vs_reference[2x7x5-all]", "test_launches_vs_reference[3x17x33-smooth05]", "test_launches_vs_reference[2x7x5-smooth05]", "test_skipped_nodes_leave_the_block_bit_equal", "test_unit_resampling_and_the_fused_entry",
        "test_refusals")] + ["tests/test_aug2d_gpu.py::" + n for n in (
        "test_launches_vs_reference", "test_exact_plans_side_by_side", "test_swap_and_single_mirrors",
        "test_integer_shift_only_plans_shift_each_section", "test_odd_section_without_swap", "test_refusals")] + [
        "tests/test_aug2d_intensity_gpu.py::" + n for n in (
        "test_batched_chain_is_the_3d_chain_of_every_draw", "test_unit_resampling", "test_refusals")] + [
        "tests/test_augin_gpu.py::" + n for n in (
        "test_launches_vs_reference[6x3x24x40-all]", "test_launches_vs_reference[2x2x17x70-all]", "test_launches_vs_reference[10x1x7x5-all]",
        "test_launches_vs_reference[3x4x20x20-all]", "test_launches_vs_reference[2x2x17x70-smooth_plane]",
        "test_launches_vs_reference[10x1x7x5-smooth_plane]", "test_skipped_nodes_leave_the_array_bit_equal", "test_every_channel_has_its_own_noise",
        "test_smoothing_of_ones_stays_in_range", "test_refusals")],
    # the target and summed-area-table tests; the trainer and driver tests of the two training files are left to "train" and NOT_USED
    "targets": [_TG + n for n in (
        "test_lsd_targets_cases", "test_lsd2d_targets_cases", "test_affinity_targets_cases", "test_affinity_targets_roi_cases",
        "test_mask_sat_cases")] + [_T2 + n for n in (
        "test_lsd2d_targets_vs_restatement", "test_lsd2d_targets_rejects_bad_input", "test_affinity_targets_roi_vs_oracle",
        "test_mask_sat_counts")] + [_TR + n for n in ("test_affinity_targets_vs_oracle", "test_lsd_targets_vs_numpy_restatement")],
    # the network's own buffers are the job of tests/guard_worker.py; here: the tensors a caller hands to it
    "unet_io": [_UN + "test_extract_block_reflect_matches_numpy_pad", _UN + "test_random_shapes_against_oracle",
                _UN + "test_lds_canary_alone_counts_no_mismatch"],
    # one training step on the smallest golden: the caller's raw, targets and weights, the views of parameters, gradients, predictions
    "train": [_TR + "test_training_step_vs_reference_goldens[affs_f4i2-f32]", _TR + "test_predictions_of_a_step_give_its_loss"],
    # the device encoders; both files put sentinels of their own behind the buffers as well.  Without the tests that go through
    # `bs predict` and the layer writer (drivers); of the 27 byte cases those at the end of a chunk, where an encoder would overrun,
    # and one of each other kind
    "blosc": [_B8 + n for n in (
        "test_one_block_chunk", "test_a_block_and_a_short_one", "test_a_chunk_of_105_bytes", "test_four_blocks_fixture_b_as_a_chunk",
        "test_overhanging_extents", "test_strided_source_and_chunk_counts", "test_more_chunks_than_one_geometry_launch_carries",
        "test_refusals")] + [_B8 + f"test_byte_cases[{c}]" for c in (
        "zeros", "noise", "far_and_near", "period300", "end14", "end13", "end12", "only1", "last1", "only12", "last13", "last300")] + [
        _B64 + "test_device_frames_decode_to_the_chunks"],
}

WHOLE = ["tests/test_synth_gpu.py", "tests/test_aug_gpu.py", "tests/test_intensity_gpu.py", "tests/test_aug2d_gpu.py",
         "tests/test_aug2d_intensity_gpu.py", "tests/test_augin_gpu.py", "tests/test_targets_gpu.py"]

_HOST = "host only: no device pointer"
_OWN = "no caller's device memory: works in its engine's own buffers, which BSMI_GUARD_MB guards (tests/test_guards_gpu.py)"
_DRIVER = "host only: chunk I/O of the drivers"

EXCLUDED = {
    "bsmi_last_error": _HOST,
    "bsmi_version": _HOST,
    "bsmi_debug_check_guards": "the checker itself; the worker calls the original at its end",
    "bsmi_debug_guard_selftest": "the checker's self-test: the worker calls it before the first family; no device pointer",
    "bsmi_debug_torch_malloc": "the allocator hook: torch calls it, not a wrapper",
    "bsmi_debug_torch_free": "the allocator hook: torch calls it, not a wrapper",
    "bsmi_debug_wino_pack_host": _HOST,
    "bsmi_agglomerate_hist_graph": _HOST,
    "bsmi_connected_components": _HOST,
    "bsmi_connected_components_multi": _HOST,
    "bsmi_mws_cluster": _HOST,
    "bsmi_rag_merge_scores_host": _HOST,
    "bsmi_rag_merge_scores_host_rule": _HOST,
    "bsmi_rag_write_sqlite": _HOST,
    "bsmi_seg_set_host_flood": "host only: a switch of the engine",
    "bsmi_stream_create_cu_mask": "host only: makes a stream",
    "bsmi_stream_destroy": "host only: destroys a stream",
    "bsmi_unet_flops": _HOST,
    "bsmi_unet_set_persistent_grid": "host only: a switch of the engine",
    "bsmi_unet_debug_activation": _OWN,
    "bsmi_unet_debug_step_info": _HOST,
    "bsmi_unet_profile_enable": "host only: the profile readers",
    "bsmi_unet_profile_read": "host only: the profile readers",
    "bsmi_unet_profile_totals": "host only: the profile readers",
    "bsmi_unet_profile_executed": "host only: the profile readers",
    "bsmi_unet_train_set_arithmetic": "host only: a switch of the engine",
    "bsmi_unet_train_set_deterministic": "host only: a switch of the engine",
    "bsmi_unet_train_adam_step": _OWN,
    "bsmi_unet_train_param_info": _HOST,
    "bsmi_unet_train_read_param": _OWN,
    "bsmi_unet_train_write_param": _OWN,
    "bsmi_unet_train_last_loss": _OWN,
    "bsmi_unet_train_grad_groups": _HOST,
    "bsmi_unet_train_wait_grad_group": "host only: waits for an event",
    "bsmi_unet_train_step_count": _HOST,
    "bsmi_unet_train_debug_tensor": _OWN,
    "bsmi_unet_train_debug_step_info": _HOST,
    "bsmi_codec_bound": _DRIVER,
    "bsmi_codec_decode": _DRIVER,
    "bsmi_codec_encode": _DRIVER,
    "bsmi_chunks_read": _DRIVER,
    "bsmi_chunks_write": _DRIVER,
    "bsmi_chunks_read_into": _DRIVER,
    "bsmi_chunks_write_from": _DRIVER,
}

NOT_USED = {
    "tests/test_redzones_gpu.py": "the guard run itself",
    "tests/test_guards_gpu.py": "the guard run of the engines' own buffers (network, training step, volume pipeline)",
    "tests/test_large_sections_gpu.py": "runs its own guard worker; full-size sections",
    "tests/test_layers_gpu.py": "the network engine's own buffers: tests/guard_worker.py",
    "tests/test_layers_edges_gpu.py": "the network engine's own buffers: tests/guard_worker.py",
    "tests/test_backward_edges_gpu.py": "the training engine's own buffers: tests/guard_worker.py",
    "tests/test_conv_below_up_gpu.py": "the network engine's own buffers; a child process per switch",
    "tests/test_fuse_up_narrow_gpu.py": "the network engine's own buffers; a child process per switch",
    "tests/test_pool_fuse_gpu.py": "the network engine's own buffers; a child process per switch",
    "tests/test_wino_in_segments_gpu.py": "the network engine's own buffers; a child process per switch",
    "tests/test_backward_gpu.py": "the training engine's own buffers: tests/guard_worker.py",
    "tests/test_wino_z_gpu.py": "the network engine's own buffers",
    "tests/test_repack_gpu.py": "the network engine's own buffers; child processes",
    "tests/test_fullsize_gpu.py": "the network engine's own buffers at full size; its segmentation half is the seg family's kernels",
    "tests/test_blosc_dev_edges_gpu.py": "the entry point is in the blosc family; this file checks bytes beyond the promised sizes with sentinels "
                                         "of its own at every edge case",
    "tests/test_drivers_gpu.py": "drivers: run_prediction / run_segmentation ask torch for allocator statistics",
    "tests/test_volume_gpu.py": "VolumePipeline asks torch for allocator statistics; two ranks",
    "tests/test_train_aug_gpu.py": "a driver (`bs train`); its kernels are the aug family's",
    "tests/test_train2d_aug_gpu.py": "a driver (`bs train`); its kernels are the aug family's",
    "tests/test_train2d_intensity_gpu.py": "a driver (`bs train`); its kernels are the aug family's",
    "tests/test_train_intensity_gpu.py": "a driver (`bs train`); its kernels are the aug family's",
    "tests/test_train_augin_gpu.py": "a driver (`bs train`); its kernels are the aug family's",
    "tests/test_train_synth_gpu.py": "a driver (`bs train`); its kernels are the synth family's",
}
