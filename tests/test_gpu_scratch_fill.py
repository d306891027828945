"""Every entry point on pre-filled scratch memory, once per family.

The library takes its device scratch from a pool that hands blocks out as they are (DevBuf::alloc, csrc/ctx.hip), and the
gridder's workspaces and the handles' own blocks straight from hipMalloc, which in practice reads as zero.  A kernel that
reads scratch it never wrote, or a host form that downloads an output block its kernels filled only in part, therefore
passes every other test: those run on fresh memory, or on blocks that a correct earlier run of the same call left behind.

Here a context of its own has the test hook "scratch_fill" (include/gridhip.h) set before its first call, so every block
it ever uses starts as 0xFF bytes (doubles NaN, ints -1, counters all-ones) or 0x01 bytes (doubles 7.7e-304, ints 16843009,
counters non-zero without being NaN - what a `!(x > 0)` test would let through).  Each row of ROWS runs one family's
smallest existing cases through that context: the functions, restatements, expected values and tolerances are those of
the family's own test module, called as they stand with the filled context in place of the session's.  Nothing is
restated or relaxed here.

The last test checks that the rows reach every entry point that include/gridhip.h declares, but for those listed in EXEMPT
with the reason why they take no scratch: a new entry point without a row fails it."""
import inspect
import sys
import time

import numpy as np
import pytest

import test_abi

pytestmark = pytest.mark.gpu

FILLS = [0xFF, 0x01]


class Recorder:
    """stands in for the ctypes library of a context: notes each symbol fetched and hands it on"""

    def __init__(self, lib, seen):
        self.__dict__["_lib"], self.__dict__["_seen"] = lib, seen

    def __getattr__(self, name):
        self._seen.add(name)
        return getattr(self._lib, name)


class Filled:
    def __init__(self, fill):
        import gridhip
        self.fill, self.seen, self.ran, self.fixtures = fill, set(), set(), {}
        self.ctx = gridhip.Context(0)
        self.ctx.set_option("scratch_fill", fill)  # before any other call: every block this context ever owns is filled
        self.ctx._lib = Recorder(self.ctx._lib, self.seen)  # before any handle is made from it: they use the context's


@pytest.fixture(scope="module", params=FILLS, ids=lambda b: f"fill{b:02X}")
def filled(request):
    f = Filled(request.param)
    yield f
    f.ctx.close()


# ---- the table -----------------------------------------------------------------------------------------------------------------
# family -> [(test module, function, its arguments but ctx and fixtures)]; arguments that need the module's own constants
# are a function of the module.  The shapes are the smallest of each test's own that still cross its internal edge.
def _wg(m):  # flag, average, ...: one work-group and one
    return dict(n=257)


ROWS = {
    "gridders": [
        ("test_gpu_coords", "test_tile_gridders_default_options", dict(H=49, Wd=33, Q=3, gh=7, gw=7)),
        ("test_gpu_coords", "test_tile_gridders_default_options", dict(H=49, Wd=33, Q=3, gh=9, gw=5)),
        ("test_gpu_coords", "test_tile_gridders_default_options", dict(H=49, Wd=33, Q=3, gh=17, gw=17)),
        ("test_gpu_coords", "test_prepass_and_coordinate_layout", dict(H=49, Wd=33, Q=3, prepass=2, layout="aligned")),
        ("test_gpu_coords", "test_prepass_and_coordinate_layout", dict(H=49, Wd=33, Q=3, prepass=1, layout="matrix")),
        ("test_gpu_coords", "test_sort_option", dict(H=49, Wd=33, Q=3, sort=2, gh=7, gw=7)),
        ("test_gpu_coords", "test_direct_variant", dict(H=49, Wd=33, Q=3, gh=7, gw=7)),
        ("test_gpu_coords", "test_grid_takes_n_from_the_height_for_both_axes", dict(H=49, Wd=33)),
        ("test_gpu_parity", "test_convgrid_and_grid", {}),
        (None, "convgrid_device_form", {}),
        ("test_gpu_parity", "test_golden_fixtures", {}),
        ("test_gpu_parity", "test_host_and_device_forms_at_the_staging_edges", dict(n=257, layout="matrix")),
        ("test_gpu_parity", "test_host_and_device_forms_at_the_staging_edges", dict(n=0, layout="columns")),
        ("test_gpu_parity", "test_two_level_prepass", dict(shape=(128, 96, 2, 2, 5, 9, 5000, {}), dist="core", mode=2)),
    ],
    "aw_gridders": [
        ("test_gpu_coords", "test_aw_gridders_on_tie_streams", dict(H=49, Wd=33, Q=3, cache=1, sort=0)),
        ("test_gpu_coords", "test_aw_gridders_on_tie_streams", dict(H=49, Wd=33, Q=3, cache=0, sort=2)),
        ("test_gpu_aw", "test_host_and_device_forms_at_the_staging_edges", dict(n=257, layout="matrix")),
        ("test_gpu_aw_degrid", "test_degrid4_matches_restatement", dict(H=40, Wd=52, W=2, Q=2, S=5, A=4, n=1500, path=1)),
        ("test_gpu_aw_degrid", "test_degrid4_matches_restatement", dict(H=64, Wd=72, W=2, Q=2, S=4, A=5, n=1000, path=3)),
        ("test_gpu_aw_degrid", "test_degrid4_overwrites_and_empty", {}),
        ("test_gpu_aw_degrid", "test_host_dev_and_sorted_general_agree", {}),
        ("test_gpu_aw_degrid", "test_plan_matches_calls", dict(n=5000)),
        ("test_gpu_aw_degrid", "test_plan_edge_cases", {}),
    ],
    "image_ops": [
        ("test_gpu_imaging", "test_wbins_and_find_closest", {}),
        ("test_gpu_imaging", "test_mirror_doweight_hermitian", {}),
        ("test_gpu_imaging", "test_centred_fft", dict(N=127)),
        ("test_gpu_imaging", "test_w_kernel", dict(npixFF=60, S=7, Q=3, w=5000.0)),
        ("test_gpu_imaging", "test_simple_and_conv_imaging", {}),
        ("test_gpu_imaging", "test_w_cache_imaging", {}),
        ("test_gpu_imaging", "test_w_cache_imaging_resident", {}),
        ("test_gpu_imaging", "test_w_kernel_table_kept_between_calls_is_never_stale", {}),
    ],
    "do_imaging": [
        ("test_gpu_imaging", "test_do_imaging", dict(kind="simple")),
        ("test_gpu_imaging", "test_do_imaging", dict(kind="conv")),
        ("test_gpu_imaging", "test_do_imaging", dict(kind="w_cache")),
        ("test_gpu_imaging", "test_do_imaging_conv_host_and_resident_at_the_staging_edges", dict(n=257, layout="matrix")),
        ("test_gpu_image_ops", "test_do_imaging_odd_n", dict(kind="w_cache", lam=180, N=9)),
        ("test_gpu_aw_imaging", "test_do_imaging_aw_resident_form", {}),
        ("test_gpu_aw_imaging", "test_aw_gridding_one_call_matches_oracle_chain", dict(lam=8000, n=3000)),
        ("test_gpu_aw_imaging", "test_doweight_order_is_pinned_per_entry_point", {}),
    ],
    "predict": [("test_gpu_predict", "test_parity_with_restatement", dict(kind=k, theta=0.1, lam=490))
                for k in ("simple", "conv", "w_cache", "aw")] +
               [("test_gpu_predict", "test_residual", dict(kind=k)) for k in ("simple", "aw")] +
               [("test_gpu_predict", "test_residual_keeps_dropped_visibilities_and_counts_them", {})] +
               [("test_gpu_predict", "test_refused_calls_leave_vis_out_untouched", {})],
    "imagers": [("test_gpu_imager", "test_against_the_calls_it_replaces", dict(kind=k, theta=0.1, lam=490))
                for k in ("simple", "conv", "w_cache", "aw")] +
               [("test_gpu_imager", "test_empty_imager", {}),
                ("test_gpu_mfs_imager", "test_spectral_psfs_and_mfs_cycle_against_the_calls_they_are_defined_by", dict(kind="w_cache")),
                ("test_gpu_mfs_imager", "test_spectral_psfs_and_mfs_cycle_against_the_calls_they_are_defined_by", dict(kind="aw")),
                ("test_gpu_weights", "test_a_weighted_imager_is_the_composition_of_existing_calls", dict(kind="simple", theta=0.1, lam=490)),
                ("test_gpu_weights", "test_a_weighted_imager_is_the_composition_of_existing_calls", dict(kind="aw", theta=0.1, lam=490))],
    "weights": [
        ("test_gpu_weights", "test_uniform_without_data_weights_is_doweight_bit_for_bit", dict(theta=0.1, lam=490)),
        ("test_gpu_weights", "test_against_the_restatement", dict(theta=0.1, lam=490, stride=3, given=True)),
        ("test_gpu_weights", "test_against_the_restatement", dict(theta=0.1, lam=640, stride=1, given=False)),
        ("test_gpu_weights", "test_in_place_and_unaligned", {}),
        ("test_gpu_weights", "test_robust_limits_and_noise_on_the_device", {}),
    ],
    "clean": [
        ("test_gpu_clean", "test_against_the_restatement", dict(N=255, gain=0.1)),
        ("test_gpu_clean", "test_host_dev_and_imager_forms_give_the_same_bits", {}),
        ("test_gpu_clean", "test_stopped_early_the_trailing_launches_are_no_ops", {}),
        ("test_gpu_clean", "test_model_is_accumulated_and_nan_is_never_selected", {}),
        ("test_gpu_clean", "test_deconvolve_is_the_loop_it_replaces", dict(kind="simple")),
        ("test_gpu_noise", "test_clean_auto_bit_for_bit", dict(N=97)),
        ("test_gpu_noise", "test_deconvolve_auto_is_the_loop_it_replaces", dict(kind="simple", scales=None)),
    ],
    "msclean": [
        ("test_gpu_msclean", "test_against_the_restatement", dict(N=97, gain=0.1)),
        ("test_gpu_msclean", "test_host_dev_and_imager_forms_give_the_same_bits", {}),
        ("test_gpu_msclean", "test_stopped_early_the_trailing_launches_are_no_ops", {}),
        ("test_gpu_msclean", "test_model_is_accumulated_and_nan_is_never_selected", {}),
        ("test_gpu_msclean", "test_deconvolve_is_the_loop_it_replaces", dict(kind="simple")),
        ("test_gpu_noise", "test_msclean_auto_against_the_restatement", dict(N=97)),
        ("test_gpu_noise", "test_masked_msclean_auto_host_dev_and_imager_forms_give_the_same_bits", {}),
        ("test_gpu_noise", "test_deconvolve_auto_is_the_loop_it_replaces", dict(kind="simple", scales=[0.0, 3.0])),
    ],
    "mfclean": [
        ("test_gpu_mfclean", "test_against_the_restatement", dict(N=255, T=2, wide_border=False, patch=0)),
        ("test_gpu_mfclean", "test_host_dev_and_imager_forms_give_the_same_bits", {}),
        ("test_gpu_mfclean", "test_stopped_early_the_trailing_launches_are_no_ops", {}),
        ("test_gpu_mfclean", "test_a_singular_hessian_changes_nothing", {}),
        ("test_gpu_mfs_imager", "test_mfdeconvolve_is_the_loop_it_replaces", {}),
    ],
    "jclean": [
        ("test_gpu_jclean", "test_against_the_restatement", dict(N=255, P=2, Q=2, metric=0, wide_border=False, patch=0)),
        ("test_gpu_jclean", "test_host_and_dev_forms_give_the_same_bits", {}),
    ],
    "image_stats": [
        ("test_gpu_noise", "test_image_stats_bit_for_bit", dict(N=257)),
        ("test_gpu_noise", "test_image_stats_bit_for_bit", dict(N=1)),
        ("test_gpu_noise", "test_image_stats_host_dev_and_imager_forms_twice", {}),
        ("test_gpu_noise", "test_image_stats_with_the_8_bit_digit", dict(N=37)),
    ],
    "automask": [
        ("test_gpu_automask", "test_labelling", lambda m: dict(N=m.automask_cases.sizes()[4])),
        ("test_gpu_automask", "test_pruning_hysteresis_growing_accumulation_and_non_finite_cells", {}),
        ("test_gpu_automask", "test_no_usable_sigma_and_nothing_taking_part", {}),
        ("test_gpu_automask", "test_host_dev_and_imager_forms_twice", {}),
        ("test_gpu_automask", "test_levels_from_image_stats_on_the_device", dict(absolute=True)),
        ("test_gpu_automask", "test_deconvolve_automask_with_nothing_above_the_level", dict(scales=None)),
        ("test_gpu_automask", "test_deconvolve_automask_is_the_loop_it_replaces", dict(scales=None)),
        ("test_gpu_automask", "test_deconvolve_automask_is_the_loop_it_replaces", dict(scales=[0.0, 3.0])),
    ],
    "noise_map": [
        ("test_gpu_noisemap", "test_bit_for_bit", dict(shape="clipped windows")),
        ("test_gpu_noisemap", "test_masks_and_invalid_nodes", {}),
        ("test_gpu_noisemap", "test_clip_rounds_on_a_bright_blob", dict(nclip=1)),
        ("test_gpu_noisemap", "test_modes_forms_null_outputs_and_in_place_twice", {}),
        ("test_gpu_noisemap", "test_automask_local_is_the_two_calls_it_replaces", {}),
    ],
    "find_sources": [
        ("test_gpu_sources", "test_patterns_bit_for_bit", lambda m: dict(N=m.automask_cases.sizes()[4])),
        ("test_gpu_sources", "test_host_dev_and_imager_forms_twice", {}),
        ("test_gpu_sources", "test_a_sky_with_a_fitted_beam_and_the_noise_from_the_device", dict(correct=True)),
        ("test_gpu_sources", "test_reasons_nothing_found_no_rows_and_an_unusable_beam", {}),
    ],
    "fit_restore": [
        ("test_gpu_restore", "test_fit_against_the_restatement", {}),
        ("test_gpu_restore", "test_restore_against_the_restatement", dict(N=255, support=8)),
        ("test_gpu_restore", "test_the_forms_give_the_same_bits_and_so_do_two_runs", {}),
        ("test_gpu_restore", "test_skipped_tiles_give_the_bits_of_the_full_sum", {}),
        ("test_gpu_restore", "test_a_failed_or_nan_beam", {}),
    ],
    "mosaic": [
        ("test_gpu_mosaic", "test_edge_shapes", dict(kind="cubic")),
        ("test_gpu_mosaic", "test_reproject_is_the_one_facet_case", {}),
        ("test_gpu_mosaic", "test_the_horizon", {}),
        ("test_gpu_mosaic", "test_weights_and_cells_that_are_not_finite", dict(kind="bilinear")),
        ("test_gpu_mosaic", "test_refused_rotations_are_counted_and_left_out_on_the_device", {}),
    ],
    "wstack": [
        ("test_gpu_wstack", "test_image_and_predict", dict(N=65, msq=(5, 9, 2), L=9)),
        ("test_gpu_wstack", "test_do_imaging_and_predict_host_and_device", dict(N=65, msq=(5, 9, 2), L=16)),
        ("test_gpu_wstack", "test_empty_middle_layer_and_partial_last_layer", {}),
        ("test_gpu_wstack", "test_a_non_finite_w_is_dropped_and_predicts_zero", {}),
        ("test_gpu_wstack", "test_too_many_layers_is_unsupported_and_an_empty_stream_is_a_zero_image", {}),
        ("test_gpu_wstack", "test_refusals_leave_the_outputs_untouched", {}),
    ],
    "dft": [
        ("test_gpu_dft", "test_parity_over_visibility_counts", lambda m: dict(n=m.WG_VIS + 1)),
        ("test_gpu_dft", "test_parity_over_component_counts", lambda m: dict(C_=m.CHUNK + 1, n=65)),
        ("test_gpu_dft", "test_parity_over_forms", {}),
        ("test_gpu_dft", "test_slices", dict(C_=7)),
        ("test_gpu_dft", "test_count_on_the_device", dict(count=3)),
        ("test_gpu_dft", "test_skipped_components", {}),
        ("test_gpu_dft", "test_non_finite_visibilities", {}),
        ("test_gpu_dft", "test_components_from_image", dict(N=33, T=3)),
        ("test_gpu_dft", "test_components_across_segments", {}),
    ],
    "gaincal": [
        ("test_gpu_gaincal", "test_every_baseline_three_intervals", dict(mode=0)),
        ("test_gpu_gaincal", "test_no_visibilities_and_no_iterations", {}),
        ("test_gpu_gaincal", "test_missing_antennas_intervals_refant_autos_and_indices_out_of_range", {}),
        ("test_gpu_gaincal", "test_around_one_chunk", lambda m: dict(n=m.CHUNK + 1)),
        ("test_gpu_gaincal", "test_lds_table_edges", dict(A=513)),
        ("test_gpu_gaincal", "test_apply_host_and_device_forms_give_the_same_bits", _wg),
        ("test_gpu_gaincal", "test_selfcal_is_predict_gaincal_apply", dict(kind="simple")),
    ],
    "ddcal": [
        ("test_gpu_ddcal", "test_every_baseline_three_intervals", dict(D=3, mode=0)),
        ("test_gpu_ddcal", "test_no_visibilities_and_no_iterations", {}),
        ("test_gpu_ddcal", "test_missing_antennas_intervals_refant_autos_and_indices_out_of_range", {}),
        ("test_gpu_ddcal", "test_around_one_chunk", lambda m: dict(n=m.CHUNK + 1)),
        ("test_gpu_ddcal", "test_subtract_host_and_device_forms_give_the_same_bits", _wg),
        ("test_gpu_ddcal", "test_peel_is_predict_ddcal_subtract_apply", dict(kind="simple")),
    ],
    "jonescal": [
        ("test_gpu_jonescal", "test_every_baseline_three_intervals", dict(mode=0)),
        ("test_gpu_jonescal", "test_no_visibilities_and_no_iterations", {}),
        ("test_gpu_jonescal", "test_missing_antennas_intervals_refant_autos_and_indices_out_of_range", {}),
        ("test_gpu_jonescal", "test_around_one_chunk", lambda m: dict(n=m.CHUNK + 1)),
        ("test_gpu_jonescal", "test_apply_host_and_device_forms_give_the_same_bits", _wg),
        ("test_gpu_jonescal", "test_stokes_is_numpy_to_the_bit", _wg),
    ],
    "flag_residuals": [
        ("test_gpu_flag", "test_either_side_of_the_path_boundary", lambda m: dict(G=m.LDS_GROUPS)),
        ("test_gpu_flag", "test_either_side_of_the_path_boundary", lambda m: dict(G=m.LDS_GROUPS + 1)),
        ("test_gpu_flag", "test_around_one_work_group", _wg),
        ("test_gpu_flag", "test_no_visibilities", {}),
        ("test_gpu_flag", "test_an_empty_group_a_small_group_and_a_normal_one", {}),
        ("test_gpu_flag", "test_rounds", {}),
        ("test_gpu_flag", "test_in_place_and_two_runs", {}),
        ("test_gpu_flag", "test_imager_form_is_predict_then_flag_residuals", dict(kind="simple")),
    ],
    "sumthreshold": [
        ("test_gpu_sumthreshold", "test_smallest_cubes", dict(shape=(2, 3, 5))),
        ("test_gpu_sumthreshold", "test_tile_edges", {}),
        ("test_gpu_sumthreshold", "test_baselines_that_are_not_thresholded_next_to_normal_ones", {}),
        ("test_gpu_sumthreshold", "test_non_finite_samples_and_bad_weights_inside_windows", {}),
        ("test_gpu_sumthreshold", "test_ladder_lengths_and_rounds", dict(K=3, niter=4)),
        ("test_gpu_sumthreshold", "test_sir_rows", dict(L=257)),
        ("test_gpu_sumthreshold", "test_the_clip_is_unchanged", {}),
    ],
    "contsub": [
        ("test_gpu_contsub", "test_rows_either_side_of_a_work_group", {}),
        ("test_gpu_contsub", "test_channels_either_side_of_a_chunk", {}),
        ("test_gpu_contsub", "test_layout_equality", {}),
        ("test_gpu_contsub", "test_clip", {}),
        ("test_gpu_contsub", "test_classes", {}),
        ("test_gpu_contsub", "test_one_row_one_channel_and_a_degenerate_coordinate", {}),
    ],
    "average": [
        ("test_gpu_average", "test_phase_shift_against_the_reference", _wg),
        ("test_gpu_average", "test_phase_shift_host_and_device_forms_give_the_same_bits", dict(n=257, stride=3)),
        ("test_gpu_average", "test_average_against_the_reference", dict(n=257, G=65)),
        ("test_gpu_average", "test_no_visibilities_and_no_group_array", {}),
        ("test_gpu_average", "test_special_values", {}),
        ("test_gpu_average", "test_the_fused_shift_is_the_two_calls", {}),
    ],
    "rm": [
        ("test_gpu_rm", "test_tables", dict(Cn=3, J=64, weighted=True)),
        # (test_tables takes the host form's table from a cache that another context may have filled: this one calls it)
        ("test_gpu_rm", "test_tables_judged_on_the_device", dict(lam2=[0.1, 0.2, 0.3], w=[1.0, -1.0, 1.0])),
        ("test_gpu_rm", "test_synth_along_m", {}),
        ("test_gpu_rm", "test_synth_bad_lines_of_sight", {}),
        ("test_gpu_rm", "test_clean_a_nan_among_good_lines_of_sight", {}),
        ("test_gpu_rm", "test_clean", dict(J=65, niter=200)),
        ("test_gpu_rm", "test_restore_and_a_model_carried_over", {}),
        ("test_gpu_rm", "test_host_and_device_forms_and_two_runs", {}),
    ],
    "fringe": [
        ("test_gpu_fringe", "test_tables", dict(F=33, T=8, tint=3, Nd=9, Nr=32)),
        ("test_gpu_fringe", "test_tables_judged_on_the_device", {}),
        ("test_gpu_fringe", "test_search_bits", dict(index=3)),
        ("test_gpu_fringe", "test_search_bits", dict(index=11)),
        ("test_gpu_fringe", "test_solve_bits", dict(refant=4, niter=50, tol=1e-9)),
        ("test_gpu_fringe", "test_fringefit_three_rounds", lambda m: dict(flag_fraction=0.3, bounds=m.FLAGGED_BOUNDS)),
        ("test_gpu_fringe", "test_apply_fringe", {}),
    ],
    "tec": [
        ("test_gpu_tec", "test_tables", dict(F=17)),
        ("test_gpu_tec", "test_tables_judged_on_the_device", {}),
        ("test_gpu_tec", "test_search_bits", dict(gi=1, fi=1)),
        ("test_gpu_tec", "test_search_bits_of_narrow_tiles", dict(Nd=65, Nm=2)),
        ("test_gpu_tec", "test_search_classes", {}),
        ("test_gpu_tec", "test_tecfit_three_rounds", lambda m: dict(flag_fraction=0.3, bounds=m.FLAGGED_BOUNDS)),
        ("test_gpu_tec", "test_apply_tec", {}),
    ],
    # the host forms' promise that a call which writes nothing, or fewer rows than the caller made room for, leaves the
    # caller's arrays as they were: the output's block must start from the caller's bytes, not from the pool's
    "refused_fringe_table": [
        ("test_gpu_fringe", "test_search_refuses_what_does_not_fit", {}),
        ("test_gpu_fringe", "test_a_table_of_another_tint_is_refused", {}),
        ("test_gpu_tec", "test_search_refuses_what_does_not_fit", {}),
    ],
    "fewer_sources_than_max_c": [(None, "fewer_sources_than_rows", {})],
}


def convgrid_device_form(ctx, oracle):
    """test_gpu_parity.test_convgrid_and_grid's case through gridhip_convgrid_dev, which no other test calls: the same
    stream, oracle and bound"""
    import test_gpu_parity as P
    from test_gpu_imager import host, to_dev
    N, Q, S, n = 128, 4, 7, 10000
    gcf, u, v, wb, vis = P.case(17, N, N, 1, Q, S, S, n)
    ref = oracle.convgrid(gcf[0], np.zeros((N, N), dtype=np.complex128), u, v, vis)
    got = ctx.convgrid(to_dev(gcf[0]), to_dev(np.zeros((N, N), dtype=np.complex128)), (to_dev(u), to_dev(v), None), to_dev(vis))
    assert P.rel(host(got), ref) < P.TOL


def fewer_sources_than_rows(ctx):
    """test_gpu_sources.check_exact makes room for two rows more than there are islands, filled with a sentinel, and
    asserts that they come back untouched: here on the cases of one image size, with and without a beam"""
    import test_gpu_sources as S
    for name, image, kw in S.box_cases(33):
        S.check_exact(ctx, name, image, dict(kw, correct=False))
    name, image, kw = S.box_cases(33)[0]
    S.check_exact(ctx, name + ", beam", image, dict(kw, correct=False), np.array([3.0, 0.5, 2.0, 0, 0, 0, 8, 1.0]))


# ---- running a row -------------------------------------------------------------------------------------------------------------
def plain(fixture):
    """the function under a @pytest.fixture"""
    get = getattr(fixture, "_get_wrapped_function", None)
    return get() if get else getattr(fixture, "__wrapped__", fixture)


def argument(f, request, mod, name):
    """what a test function's parameter `name` gets here: the filled context, the session's oracle and golden files, or the
    value of the module's own fixture of that name (made once per filled context, with the filled context)"""
    if name == "ctx":
        return f.ctx
    if name in ("oracle", "golden"):
        return request.getfixturevalue(name)
    key = (mod.__name__, name)
    if key not in f.fixtures:
        fn = plain(getattr(mod, name))
        assert not inspect.isgeneratorfunction(fn), f"{key}: a fixture with a teardown has no place in this table"
        f.fixtures[key] = fn(*(argument(f, request, mod, p) for p in inspect.signature(fn).parameters))
    return f.fixtures[key]


def run_case(f, request, module, function, kwargs):
    mod = sys.modules[__name__] if module is None else __import__(module)
    fn = getattr(mod, function)
    kwargs = dict(kwargs(mod) if callable(kwargs) else kwargs or {})
    for name in inspect.signature(fn).parameters:
        if name not in kwargs:
            kwargs[name] = argument(f, request, mod, name)
    fn(**kwargs)


def run_row(f, request, family):
    ctx = f.ctx
    before = ctx.get_option("scratch_filled")
    for module, function, kwargs in ROWS[family]:
        t0 = time.perf_counter()
        run_case(f, request, module, function, kwargs)
        ctx.synchronize()
        print(f"  {family}: {module}.{function} {time.perf_counter() - t0:.2f} s", file=sys.stderr)
    assert ctx.get_option("scratch_filled") > before, "the row drew no block: it proves nothing"
    assert ctx.get_option("errors") == 0
    assert ctx.get_option("scratch_fill") == f.fill


@pytest.mark.parametrize("reuse", ["reuse_on", "reuse_off"])
@pytest.mark.parametrize("family", ["gridders", "aw_gridders"])
def test_gridders(filled, request, family, reuse):
    """the gridders keep records and sorted lists between calls ("bin_reuse", "list_reuse"): a row with both at their
    default, and one with both off"""
    off = 1 if reuse == "reuse_off" else 0
    filled.ctx.set_option("bin_reuse", off)
    filled.ctx.set_option("list_reuse", off)
    try:
        run_row(filled, request, family)
    finally:
        filled.ctx.set_option("bin_reuse", 0)
        filled.ctx.set_option("list_reuse", 0)
    filled.ran.add((family, reuse))


FAMILIES = [f for f in ROWS if f not in ("gridders", "aw_gridders")]


@pytest.mark.parametrize("family", FAMILIES)
def test_family(filled, request, family):
    run_row(filled, request, family)
    filled.ran.add(family)


def test_the_hook_itself(filled):
    """the option reads back and refuses what is no byte; the count is read-only and rises with the blocks of a call"""
    import gridhip
    ctx = filled.ctx
    assert ctx.get_option("scratch_fill") == filled.fill
    for bad in (256, 1 << 40):
        with pytest.raises(gridhip.GridHipError) as e:
            ctx.set_option("scratch_fill", bad)
        assert e.value.code == gridhip._lib.EINVAL and ctx.get_option("scratch_fill") == filled.fill
    with pytest.raises(gridhip.GridHipError):
        ctx.set_option("scratch_filled", 0)  # read-only
    before = ctx.get_option("scratch_filled")
    img = np.arange(25.0).reshape(5, 5)
    st = ctx.image_stats(img, None, 0)  # one staged input, one staged output, one scratch block
    assert ctx.get_option("scratch_filled") >= before + 3 and np.all(np.isfinite(st[:4]))


# ---- the coverage check ----------------------------------------------------------------------------------------------------------
_COMM = "the communicator family makes contexts of its own per device and needs RCCL set up in a process of its own: " \
        "seconds per case on one GPU (tests/test_gpu_distributed.py runs it in child processes)"
EXEMPT = {
    "gridhip_version": "a constant",
    "gridhip_strerror": "a string table",
    "gridhip_device_count": "asks the runtime; no context",
    "gridhip_create": "makes the context: nothing can be filled before it",
    "gridhip_destroy": "frees the context's blocks",
    "gridhip_last_error": "returns the context's message",
    "gridhip_set_stream": "orders two streams with an event",
    "gridhip_reset_stream": "orders two streams with an event",
    "gridhip_get_stream": "returns a field",
    "gridhip_synchronize": "waits for the stream",
    "gridhip_set_option": "writes a host field",
    "gridhip_get_option": "reads a host field or d_scalars",
    "gridhip_last_dropped": "reads d_scalars",
    "gridhip_last_timing": "reads events",
    "gridhip_timing": "reads events",
    "gridhip_enable_timing": "writes host fields",
    "gridhip_aw_last_stats": "reads d_scalars",
    "gridhip_image_size": "arithmetic on its arguments",
    "gridhip_noise_map_nodes": "arithmetic on its arguments",
    "gridhip_ddcal_lds_antennas": "arithmetic on its argument",
    "gridhip_jonescal_lds_antennas": "a constant",
    "gridhip_sumthreshold_tile": "constants",
    "gridhip_rm_tile": "constants",
    "gridhip_contsub_tile": "constants",
    "gridhip_fringe_tile": "constants",
    "gridhip_tec_tile": "constants",
    "gridhip_malloc": "the caller's memory: hipMalloc, not the pool",
    "gridhip_free": "the caller's memory",
    "gridhip_memcpy_h2d": "a copy between the caller's arrays",
    "gridhip_memcpy_d2h": "a copy between the caller's arrays",
    "gridhip_memset": "a memset of the caller's array",
    "gridhip_plan_destroy": "frees the plan's blocks",
    "gridhip_aw_plan_destroy": "frees the plan's blocks",
    "gridhip_imager_destroy": "frees the imager's blocks",
    "gridhip_wstack_destroy": "frees the stack's blocks",
    "gridhip_wstack_info": "returns host fields of the stack",
}
EXEMPT.update({s: _COMM for s in test_abi.declared_symbols() if s.startswith("gridhip_comm_")})


def test_every_entry_point_has_a_row(filled):
    every = {(fam, r) for fam in ("gridders", "aw_gridders") for r in ("reuse_on", "reuse_off")} | set(FAMILIES)
    if filled.ran != every:
        pytest.skip(f"{len(every - filled.ran)} rows of the table did not run (or fail) in this session: nothing to conclude")
    declared = set(test_abi.declared_symbols())
    assert set(EXEMPT) <= declared, sorted(set(EXEMPT) - declared)
    assert all(isinstance(r, str) and r for r in EXEMPT.values())
    missing = sorted(declared - set(EXEMPT) - filled.seen)
    assert not missing, f"entry points no row of ROWS reaches under scratch_fill: {missing}"
