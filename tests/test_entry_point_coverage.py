"""Ledger of the C ABI: every entry point include/fsv2v.h declares names the operator-level check that drives it directly
(through lib.call, against a CPU reference, on the emulator and on the GPU), or says why it has none.  A new entry point
without a line here fails this module: write its check first.

The table was produced on the emulator by recording the entry points lib.call / lib.call_status issued while the check
modules ran (op_checks, small_op_checks, h_checks, np_checks, spade_k3_checks, adaptive_conv_checks, tile_checks,
weight_path_checks, attn_fused_checks, attn_fused_grad_checks).  Calls made
under the whole-iteration functions of those modules (check_step, check_inference: one D + G step or a full inference, compared
through losses and gradient norms) do not count.  Where several checks reach an entry point, small_op_checks, then op_checks,
come first, and within a module the check that calls it most often.  Nothing is launched here."""
import importlib
import re

from test_abi import declared_symbols

HOST_ONLY = "host-only"          # measurement-only and planning entry points: nothing to compare with a reference
_HOST_ONLY_NAMES = re.compile(r"^fsv_stamp|_plan$|_rule$|_info$|_supported$|_workspace_doubles$|_scratch_floats$")

CHECKED_BY = {
    'fsv_act_bwd':                     'op_checks.check_conv',
    'fsv_act_fwd':                     'small_op_checks.check_act_fwd',
    'fsv_adam_step':                   'small_op_checks.check_adam_fp64',
    'fsv_adam_step_range':             'small_op_checks.check_adam_ranges',
    'fsv_adaptive_avgpool_bwd':        'op_checks.check_adaptive_avgpool',
    'fsv_adaptive_avgpool_fwd':        'op_checks.check_adaptive_avgpool',
    'fsv_amp_adam':                    'small_op_checks.check_amp_adam',
    'fsv_amp_check':                   'small_op_checks.check_amp_check',
    'fsv_amp_update':                  'small_op_checks.check_amp_update',
    'fsv_attention_fused_bwd':         'attn_fused_grad_checks.check_bounds',
    'fsv_attention_fused_bwd_plan':    'host-only',
    'fsv_attention_fused_fwd':         'attn_fused_checks.check_splits',
    'fsv_attention_fused_fwd_lse':     'attn_fused_grad_checks.check_forward_lse',
    'fsv_attention_fused_plan':        'host-only',
    'fsv_avgpool3s2_bwd':              'op_checks.check_avgpool3s2',
    'fsv_avgpool3s2_fwd':              'op_checks.check_avgpool3s2',
    'fsv_bias_act':                    'small_op_checks.check_bias_act',
    'fsv_bilinear_resize_fwd':         'op_checks.check_flownet_ops',
    'fsv_blend_bwd':                   'small_op_checks.check_blend_bwd',
    'fsv_blend_fwd':                   'op_checks.check_warp_compose',
    'fsv_cast_half':                   'op_checks.check_spade',
    'fsv_cat_get':                     'op_checks.check_cat_and_pad',
    'fsv_cat_put':                     'op_checks.check_cat_and_pad',
    'fsv_channelnorm_fwd':             'op_checks.check_flownet_ops',
    'fsv_colsum':                      'small_op_checks.check_two_launch_reductions',
    'fsv_colsum_fused':                'op_checks.check_spade',
    'fsv_colsum_grouped':              'op_checks.check_conv',
    'fsv_colsum_plan':                 'host-only',
    'fsv_conv_gather_fwd':             'op_checks.check_conv',
    'fsv_conv_gather_fwd_np':          'np_checks.check_forward',
    'fsv_conv_gather_fwd_stats':       'op_checks.check_conv_stats',
    'fsv_conv_gather_group':           'op_checks.check_conv',
    'fsv_conv_group_plan':             'host-only',
    'fsv_conv_plan':                   'host-only',
    'fsv_conv_thin_rule':              'host-only',
    'fsv_conv_tile_info':              'host-only',
    'fsv_conv_wgrad':                  'op_checks.check_conv',
    'fsv_conv_wgrad_group':            'op_checks.check_conv_groups',
    'fsv_conv_wgrad_np':               'np_checks.check_wgrad',
    'fsv_correlation_fwd':             'op_checks.check_flownet_ops',
    'fsv_crop_resize_bwd':             'op_checks.check_face_ops',
    'fsv_crop_resize_fwd':             'op_checks.check_face_ops',
    'fsv_face_boxes':                  'op_checks.check_face_ops',
    'fsv_gather_add':                  'small_op_checks.check_gather_add',
    'fsv_hconv_gather':                'op_checks.check_spade',
    'fsv_hconv_plan':                  'host-only',
    'fsv_hconv_prep_weight':           'h_checks.check_prep_weight_tables',
    'fsv_hconv_prep_weight_one':       'op_checks.check_spade',
    'fsv_hconv_wgrad':                 'op_checks.check_spade',
    'fsv_hinge_bwd':                   'op_checks.check_losses',
    'fsv_hinge_fwd':                   'op_checks.check_loss_reductions',
    'fsv_l1_bwd':                      'op_checks.check_losses',
    'fsv_l1_fwd':                      'op_checks.check_loss_reductions',
    'fsv_maxpool2_bwd':                'small_op_checks.check_maxpool2',
    'fsv_maxpool2_fwd':                'small_op_checks.check_maxpool2',
    'fsv_norm_apply':                  'small_op_checks.check_sync_bn',
    'fsv_norm_bwd':                    'small_op_checks.check_two_launch_reductions',
    'fsv_norm_bwd_apply':              'small_op_checks.check_sync_bn',
    'fsv_norm_bwd_fused':              'small_op_checks.check_sync_bn',
    'fsv_norm_bwd_sums':               'small_op_checks.check_sync_bn',
    'fsv_norm_stats':                  'small_op_checks.check_two_launch_reductions',
    'fsv_norm_stats_finish':           'op_checks.check_conv_stats',
    'fsv_norm_stats_from_sums':        'small_op_checks.check_sync_bn',
    'fsv_norm_stats_fused':            'op_checks.check_spade',
    'fsv_norm_stats_rep':              'small_op_checks.check_two_launch_reductions',
    'fsv_norm_sums':                   'small_op_checks.check_sync_bn',
    'fsv_norm_workspace_doubles':      'host-only',
    'fsv_pack_d_x':                    'op_checks.check_losses',
    'fsv_pad_channels':                'op_checks.check_conv',
    'fsv_pad_channels_h':              'op_checks.check_cat_and_pad',
    'fsv_part_masks':                  'op_checks.check_part_masks',
    'fsv_paste_face_bwd':              'op_checks.check_face_ops',
    'fsv_paste_face_fwd':              'op_checks.check_face_ops',
    'fsv_pool15':                      'op_checks.check_losses',
    'fsv_pool_rows_bwd':               'adaptive_conv_checks.check_pool_windows',
    'fsv_pool_rows_fwd':               'adaptive_conv_checks.check_pool_windows',
    'fsv_prep_weight':                 'weight_path_checks.check_prep_weight_modes',
    'fsv_prep_weight_grouped':         'weight_path_checks.check_layouts',
    'fsv_resample2d_fwd':              'op_checks.check_flownet_ops',
    'fsv_sn_backward':                 'weight_path_checks.check_sn_backward',
    'fsv_sn_power_iter':               'weight_path_checks.check_power_iteration',
    'fsv_sn_power_iter_batched':       'weight_path_checks.check_power_iteration_batched',
    'fsv_sn_scratch_floats':           'host-only',
    'fsv_softmax_rows_bwd':            'op_checks.check_softmax',
    'fsv_softmax_rows_fwd':            'op_checks.check_softmax',
    'fsv_spade_bwd_elem':              'op_checks.check_spade',
    'fsv_spade_conv3_fwd':             'op_checks.check_spade_conv3',
    'fsv_spade_conv3_supported':       'host-only',
    'fsv_spade_conv_s_fwd':            'op_checks.check_spade_conv_s',
    'fsv_spade_conv_s_fwd_h':          'op_checks.check_spade_conv_s',
    'fsv_spade_conv_s_supported':      'host-only',
    'fsv_spade_k3_fwd':                'spade_k3_checks.check_op',
    'fsv_spade_mod_bwd':               'op_checks.check_spade',
    'fsv_spade_mod_bwd_h':             'op_checks.check_spade',
    'fsv_spade_mod_fwd':               'op_checks.check_spade',
    'fsv_spade_mod_fwd_h':             'op_checks.check_spade',
    'fsv_spade_prep':                  'op_checks.check_spade',
    'fsv_spade_prep_h':                'op_checks.check_spade',
    'fsv_stamp':                       'host-only',
    'fsv_stamp_rate_khz':              'host-only',
    'fsv_sum_terms':                   'small_op_checks.check_sum_terms',
    'fsv_unpack_d_grad':               'op_checks.check_losses',
    'fsv_unpack_d_grad_h':             'h_checks.check_unpack_d_grad_h',
    'fsv_upload_i64':                  'small_op_checks.check_upload_i64',
    'fsv_upsample2x_bwd':              'op_checks.check_conv_up',
    'fsv_upsample2x_fwd':              'op_checks.check_conv_up',
    'fsv_warp_bwd':                    'op_checks.check_warp',
    'fsv_warp_compose_bwd':            'op_checks.check_warp_compose',
    'fsv_warp_compose_fwd':            'op_checks.check_warp_compose',
    'fsv_warp_fwd':                    'op_checks.check_warp',
    'fsv_wgrad_finalize':              'weight_path_checks.check_finalize',
    'fsv_wsum_bwd':                    'op_checks.check_weighted_sum',
    'fsv_wsum_fwd':                    'op_checks.check_weighted_sum',
}

# Entry points the operator-level checks do not reach yet, with where the suite does reach them.  This set may only shrink.
NO_DIRECT_CHECK = {
    'fsv_pack_d_input': "no call site in the package any more (fsv_pack_d_x replaced it)",
    'fsv_pack_d_single': "no call site in the package any more (fsv_pack_d_x replaced it)",
}


def test_every_entry_point_is_in_the_ledger():
    declared = set(declared_symbols())
    assert not set(CHECKED_BY) & set(NO_DIRECT_CHECK)
    listed = set(CHECKED_BY) | set(NO_DIRECT_CHECK)
    assert listed == declared, (sorted(declared - listed), sorted(listed - declared))
    assert len(NO_DIRECT_CHECK) <= 2 and all(len(reason) > 20 for reason in NO_DIRECT_CHECK.values())


def test_only_planning_and_measurement_entry_points_are_host_only():
    bad = [name for name, check in CHECKED_BY.items() if check == HOST_ONLY and not _HOST_ONLY_NAMES.search(name)]
    assert not bad, bad


def test_every_named_check_exists():
    missing = []
    for name, check in sorted(CHECKED_BY.items()):
        if check == HOST_ONLY:
            continue
        module, _, fn = check.partition('.')
        if not callable(getattr(importlib.import_module(module), fn, None)):
            missing.append((name, check))
    assert not missing, missing
