"""ctypes binding of libecm_hip.so (the C ABI declared in include/ecm_hip.h and, for the geometry, rectification, temporal and
motion, volume, mesh, colour and augmentation entries, include/ecm_geometry.h, include/ecm_rectify.h, include/ecm_temporal.h,
include/ecm_motion.h, include/ecm_volume.h, include/ecm_mesh.h, include/ecm_color.h and include/ecm_augment.h).

The product path has NO fallback: if the library is missing or a call fails, a RuntimeError is
raised.  Each table below mirrors its header one to one: tests/test_abi_types.py parses every header of TABLES and compares
every return type and every parameter type, in order, and the names with the built library's exports; and
tests/test_hip_abi_calls.py checks the values that ops.py hands to them on the device.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ECM_HIP_LIB") or os.path.join(_HERE, "csrc", "libecm_hip.so")    # ECM_HIP_LIB: an experiment build

_P, _I, _LL, _F = C.c_void_p, C.c_int, C.c_longlong, C.c_float

# name -> (restype, argtypes); the single source of truth for the Python side of the ABI
PROTOTYPES = {
    "ecm_abi_version": (_I, []),
    "ecm_error_string": (C.c_char_p, [_I]),
    "ecm_costvol_concat_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ecm_costvol_concat_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ecm_softargmin_heads_fwd": (_I, [_P, _LL, _P, _I, _I, _I, _I, _P]),
    "ecm_softargmin_heads_lse_fwd": (_I, [_P, _LL, _P, _P, _I, _I, _I, _I, _P]),
    "ecm_softargmin_heads_bwd": (_I, [_P, _LL, _P, _P, _I, _I, _I, _I, _P]),
    "ecm_disparity_regression_fwd": (_I, [_P, _P, _I, _I, _I, _P]),
    "ecm_aggregate9_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ecm_aggregate9_stats_fwd": (_I, [_P, _LL, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "ecm_aggregate9_mode_fwd": (_I, [_P, _LL, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ecm_aggregate9_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ecm_weights9_scratch_bytes": (_LL, [_I, _I, _I]),
    "ecm_weights9_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _LL, _I, _I, _I, _I, _P]),
    "ecm_context_weights_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _LL, _I, _I, _I, _I, _I, _P]),
    "ecm_context_weights_bwd_scratch_bytes": (_LL, [_I, _I, _I, _I, _I]),
    "ecm_context_weights_bwd": (_I, [_P] * 11 + [_P, _LL, _I, _I, _I, _I, _I, _P]),
    "ecm_volume_mapping_fwd": (_I, [_P, _LL, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "ecm_trilinear_softargmin_fwd": (_I, [_P, _LL, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ecm_volume_mapping_stats_fwd": (_I, [_P, _LL, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "ecm_trilinear_softargmin_stats_fwd": (_I, [_P, _LL, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ecm_volume_mapping_mode_fwd": (_I, [_P, _LL, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ecm_trilinear_softargmin_mode_fwd": (_I, [_P, _LL, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ecm_volume_mapping_bwd_scratch_bytes": (_LL, [_I] * 6),
    "ecm_volume_mapping_bwd": (_I, [_P, _LL, _P, _P, _P, _P, _P, _P, _P, _LL, _I, _I, _I, _I, _I, _I, _P]),
    "ecm_trilinear_softargmin_bwd_scratch_bytes": (_LL, [_I] * 7),
    "ecm_trilinear_softargmin_bwd": (_I, [_P, _LL, _P, _P, _P, _LL, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ecm_weights9_bwd_scratch_bytes": (_LL, [_I, _I, _I, _I]),
    "ecm_weights9_bwd": (_I, [_P] * 11 + [_P, _LL, _I, _I, _I, _I, _P]),
    "ecm_conv3d_packed_floats": (_LL, [_I, _I]),
    "ecm_conv3d_pack_weight": (_I, [_P, _P, _I, _I, _I, _P]),
    "ecm_conv3d_k3_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ecm_conv_wino_packed_floats": (_LL, [_I, _I, _I]),
    "ecm_conv_wino_pack_weight": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "ecm_conv_wino_pack_weight2": (_I, [_P, _P, _I, _I, _I, _P]),
    "ecm_conv_wino_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ecm_conv_wino_fwd_add": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ecm_sum_n": (_I, [_P, _P, _P, _P, _P, _LL, _P]),
    "ecm_zero_insert2d": (_I, [_P, _P, _LL, _I, _I, _I, _I, _P]),
    "ecm_costvol_class_weights_fwd": (_I, [_P, _P, _P, _I, _I, _P]),
    "ecm_costvol_class_weights_bwd": (_I, [_P, _P, _P, _I, _I, _P]),
    "ecm_conv_wino_wgrad_scratch_bytes": (_LL, [_I] * 7),
    "ecm_conv_wino_wgrad": (_I, [_P, _P, _P, _P, _LL] + [_I] * 7 + [_P]),
    "ecm_conv3d_c1_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ecm_conv3d_c1_dgrad": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ecm_conv3d_c1_wgrad_scratch_bytes": (_LL, [_I, _I, _I, _I, _I]),
    "ecm_conv3d_c1_wgrad": (_I, [_P, _P, _P, _P, _LL, _I, _I, _I, _I, _I, _P]),
    "ecm_conv3d_c1_gn_fwd": (_I, [_P] * 6 + [_I, _I, _I, _I, _I, _P]),
    "ecm_conv3d_c1_gn_wgrad": (_I, [_P] * 7 + [_LL, _I, _I, _I, _I, _I, _P]),
    "ecm_deconv3d_pack_weight": (_I, [_P, _P, _I, _I, _P]),
    "ecm_deconv3d_k3s2_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ecm_conv3d_wgrad_scratch_bytes": (_LL, [_I, _I, _I, _I, _I, _I, _I]),
    "ecm_conv3d_k3_wgrad": (_I, [_P, _P, _P, _P, _LL, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ecm_conv2d_packed_floats_ex": (_LL, [_I] * 4),
    "ecm_conv2d_pack_weight_ex": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "ecm_conv2d_fwd_ex": (_I, [_P, _P, _P] + [_I] * 13 + [_P]),
    "ecm_conv2d_wgrad_ex_scratch_bytes": (_LL, [_I] * 8),
    "ecm_conv2d_wgrad_ex": (_I, [_P, _P, _P, _P, _LL] + [_I] * 13 + [_P]),
    "ecm_deconv2d_pack_weight": (_I, [_P, _P, _I, _I, _P]),
    "ecm_deconv2d_k3s2_fwd": (_I, [_P, _P, _P] + [_I] * 7 + [_P]),
    "ecm_deconv2d_k3s2_bias_fwd": (_I, [_P, _P, _P, _P] + [_I] * 7 + [_P]),
    "ecm_channel_sum_scratch_bytes": (_LL, [_I, _I, _LL]),
    "ecm_channel_sum": (_I, [_P, _P, _P, _LL, _I, _I, _LL, _P]),
    "ecm_conv2d_c1_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "ecm_conv2d_c1_dgrad": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "ecm_conv2d_c1_wgrad_scratch_bytes": (_LL, [_I, _I, _I, _I]),
    "ecm_conv2d_c1_wgrad": (_I, [_P, _P, _P, _P, _P, _P, _LL, _I, _I, _I, _I, _P]),
    "ecm_stereo_loss_scratch_bytes": (_LL, [_LL]),
    "ecm_stereo_loss_fwd": (_I, [_P] * 6 + [_LL, _LL, _F, _F, _F, _F, _P]),
    "ecm_stereo_loss_bwd": (_I, [_P] * 9 + [_LL, _F, _F, _F, _F, _P]),
    "ecm_costvol_conv_assemble_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ecm_costvol_conv_assemble_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ecm_frame_prep": (_I, [_P] * 5 + [_I, _I, _I, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "ecm_frame_prep_kitti_eval": (_I, [_P] * 5 + [_I, _I, _I, _I, _I, _P, _P, _P]),
    "ecm_frame_prep_packed": (_I, [_P, _P, _I] + [_P] * 4 + [_I, _I, _I, _P, _P, _I, _I, _I, _I, _P, _P, _I, _P]),
    "ecm_eval_epe_scratch_bytes": (_LL, [_LL]),
    "ecm_eval_epe": (_I, [_P, _P, _P, _P, _LL] + [_I] * 7 + [_F, _P]),
    "ecm_eval_kitti_scratch_bytes": (_LL, [_I, _I, _I]),
    "ecm_eval_kitti": (_I, [_P, _P, _P, _P, _P, _LL, _I, _I, _I, _F, _P]),
    "ecm_eval_sparsify_max_measures": (_I, []),
    "ecm_eval_sparsify_max_steps": (_I, []),
    "ecm_eval_sparsify_scratch_bytes": (_LL, [_I] * 5),
    "ecm_eval_sparsify": (_I, [_P, _P, _P, _P, _P, _P, _LL, _I, _I, _I, _I, _I, _F, _P]),
    "ecm_disp_to_u16": (_I, [_P, _P, _I, _I, _I, _P, _P, _I, _I, _F, _P]),
    "ecm_lr_check_max_width": (_I, []),
    "ecm_lr_check_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _F, _F, _I, _P]),
    "ecm_disp_filter_max_radius": (_I, [_I]),
    "ecm_disp_median_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "ecm_disp_bilateral_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _F, _P]),
    "ecm_disp_speckle_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _F, _P]),
    "ecm_disp_wls_scratch_bytes": (_LL, [_I, _I, _I]),
    "ecm_disp_wls_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _F, _I, _P]),
    "ecm_disp_splat_max_width": (_I, []),
    "ecm_disp_splat_fwd": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "ecm_gn3d_cluster_mode": (_I, [_I]),
    "ecm_gn3d_poll_ms": (_I, [_I]),
    "ecm_async_status": (_I, [_I]),
    "ecm_gn3d_scratch_bytes": (_LL, [_I, _I, _LL]),
    "ecm_gn3d_stats": (_I, [_P, _P, _P, _LL, _I, _I, _LL, _F, _P]),
    "ecm_gn3d_apply": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _LL, _I, _P]),
    "ecm_gn3d_fwd": (_I, [_P] * 7 + [_LL, _I, _I, _LL, _I, _F, _P]),
    "ecm_gn3d_bwd": (_I, [_P] * 11 + [_LL, _I, _I, _LL, _I, _P]),
    "ecm_gn3d_cluster_bytes": (_LL, [_I]),
    "ecm_gn3d_cluster_preset": (_I, [_P, _LL, _P]),
    "ecm_gn3d_fwd_p": (_I, [_P] * 7 + [_LL, _P, _LL, _I, _I, _LL, _I, _F, _P]),
    "ecm_gn3d_bwd_p": (_I, [_P] * 11 + [_LL, _P, _LL, _I, _I, _LL, _I, _P]),
    "ecm_conv3d_bf16_packed_elems": (_LL, [_I, _I]),
    "ecm_conv3d_bf16_pack_weight": (_I, [_P, _P, _I, _I, _I, _P]),
    "ecm_conv3d_k3_bf16_fwd": (_I, [_P, _P, _P] + [_I] * 7 + [_P]),
    "ecm_deconv3d_k3s2_bf16_fwd": (_I, [_P, _P, _P] + [_I] * 6 + [_P]),
    "ecm_gn3d_stats_bf16": (_I, [_P, _P, _P, _LL, _I, _I, _LL, _F, _P]),
    "ecm_gn3d_apply_bf16": (_I, [_P] * 6 + [_I, _I, _LL, _I, _P]),
    "ecm_gn3d_apply_f32_bf16": (_I, [_P] * 6 + [_I, _I, _LL, _I, _P]),
    "ecm_conv3d_c1_gn_fwd_bf16": (_I, [_P] * 6 + [_I, _I, _I, _I, _I, _P]),
    "ecm_conv2d_bf16_packed_elems": (_LL, [_I, _I, _I]),
    "ecm_conv2d_bf16_pack_weight": (_I, [_P, _P, _I, _I, _I, _P]),
    "ecm_conv2d_bf16_fwd": (_I, [_P, _P, _P] + [_I] * 9 + [_P]),
    "ecm_gn3d_apply_bf16_f32": (_I, [_P] * 7 + [_I, _I, _LL, _I, _P]),
    "ecm_deconv2d_bf16_packed_elems": (_LL, [_I, _I]),                       # cmf.py:236-239
    "ecm_deconv2d_bf16_pack_weight": (_I, [_P, _P, _I, _I, _P]),             # cmf.py:236-239
    "ecm_deconv2d_k3s2_bias_bf16_fwd": (_I, [_P, _P, _P, _P] + [_I] * 5 + [_P]),   # cmf.py:236-239
    "ecm_conv2d_c1_bf16_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),    # cmf.py:259-264
    "ecm_conv3d_split_packed_elems": (_LL, [_I, _I]),                        # cmfsm.py:244-268
    "ecm_conv3d_split_pack_weight": (_I, [_P, _P, _I, _I, _I, _P]),          # cmfsm.py:244-268
    "ecm_conv3d_k3s2_split_fwd": (_I, [_P, _P, _P] + [_I] * 6 + [_P]),       # cmfsm.py:244-258
    "ecm_deconv3d_k3s2_split_fwd": (_I, [_P, _P, _P] + [_I] * 9 + [_P]),     # cmfsm.py:262-268
}

# The geometry entries (include/ecm_geometry.h, prefix ecmg_): a table of their own.  PROTOTYPES stays the image of
# include/ecm_hip.h (the network and its post-filters); call(), query() and missing_symbols() serve every table of TABLES.
GEOMETRY_PROTOTYPES = {
    "ecmg_reproject_fwd": (_I, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _F, _F, _P]),
    "ecmg_point_cloud_tile": (_I, []),
    "ecmg_point_cloud_scratch_bytes": (_LL, [_I, _I, _I]),
    "ecmg_point_cloud_fwd": (_I, [_P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _LL, _I, _I, _I, _F, _F, _P]),
}

# The rectification entries (include/ecm_rectify.h, prefix ecmr_): a third table.
RECTIFY_PROTOTYPES = {
    "ecmr_rectify_map_params": (_I, []),
    "ecmr_tile_width": (_I, []),
    "ecmr_rectify_map_fwd": (_I, [_P, _P, _I, _I, _P]),
    "ecmr_remap_pair_fwd": (_I, [_P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _F, _P]),
}


# header file under include/ -> (its table, the prefix its names bear): the registry that load(), missing_symbols() and the census
# of tests/test_abi_types.py go through.  The values ARE the three dicts above (tests mutate them in place); a fourth header is a
# fourth row here and nothing else.
TABLES = {
    "ecm_hip.h": (PROTOTYPES, "ecm_"),
    "ecm_geometry.h": (GEOMETRY_PROTOTYPES, "ecmg_"),
    "ecm_rectify.h": (RECTIFY_PROTOTYPES, "ecmr_"),
}


# The temporal entries (include/ecm_temporal.h, prefix ecmt_): the warp of a disparity map to the next frame and its fusion.
TEMPORAL_PROTOTYPES = {
    "ecmt_disparity_warp_max_attributes": (_I, []),
    "ecmt_disparity_warp_scratch_bytes": (_LL, [_I, _I, _I]),
    "ecmt_disparity_warp_fwd": (_I, [_P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _LL, _I, _I, _I, _F, _F, _I, _P]),
    "ecmt_disparity_fuse_fwd": (_I, [_P] * 9 + [_LL, _F, _F, _I, _P]),
}

# A second registry, of the same form as TABLES, for headers added after the census of tests/test_abi_types.py and
# tests/test_abi_refusals.py was closed over the three rows above: those files spell the headers out, so a row added to TABLES
# has to arrive together with an edit of them.  load(), missing_symbols(), call() and query() serve both registries alike, and the
# new header's own test file holds it to the same census.  Folding this row into TABLES, and its rows into the census files, is
# a later change that may touch them.
EXTENSION_TABLES = {
    "ecm_temporal.h": (TEMPORAL_PROTOTYPES, "ecmt_"),
}


# The motion entries (include/ecm_motion.h, prefix ecmm_): the normal equations of the dense disparity alignment.
MOTION_PROTOTYPES = {
    "ecmm_align_sums": (_I, []),
    "ecmm_align_scratch_bytes": (_LL, [_I, _I, _I, _I]),
    "ecmm_align_normal_fwd": (_I, [_P] * 8 + [_I, _P, _P, _P, _LL, _I, _I, _I, _I, _F, _F, _F, _F, _F, _P]),
}

# A third registry of the same form: tests/test_disp_warp_cpu.py pins the keys of TABLES (three rows) and of EXTENSION_TABLES
# (ecm_temporal.h alone), so a fifth header can be a row of neither without an edit of that file.  Its own test file holds it to
# the same census.  Folding the three registries into one is a later change that may touch the census files.
MOTION_TABLES = {
    "ecm_motion.h": (MOTION_PROTOTYPES, "ecmm_"),
}

# every registry that load(), missing_symbols(), call() and query() serve
REGISTRIES = (TABLES, EXTENSION_TABLES, MOTION_TABLES)


def _tables():
    return [row for registry in REGISTRIES for table, _ in registry.values() for row in table.items()]


# The volume entries (include/ecm_volume.h, prefix ecmv_): the TSDF volume's integration and raycast.
VOLUME_PROTOTYPES = {
    "ecmv_integrate_fwd": (_I, [_P] * 8 + [_I] * 7 + [_F] * 4 + [_P]),
    "ecmv_raycast_max_steps": (_I, []),
    "ecmv_raycast_fwd": (_I, [_P] * 4 + [_I, _P, _P] + [_I] * 6 + [_F, _F, _F, _I, _P]),
}

VOLUME_TABLES = {
    "ecm_volume.h": (VOLUME_PROTOTYPES, "ecmv_"),
}

# tests/test_motion_align_cpu.py pins len(REGISTRIES) == 3 and the row count of _tables() to REGISTRIES, so a sixth header can be a
# row of none of the three without an edit of that file.  The registries added after that census was closed are listed here:
# load() and missing_symbols() walk _tables() and these, so call() and query() serve them alike, and the new header's own test
# file holds it to the same census.  Folding everything into one registry is a later change that may touch the census files.
LATER_REGISTRIES = (VOLUME_TABLES,)


def _all_tables():
    return _tables() + [row for registry in LATER_REGISTRIES for table, _ in registry.values() for row in table.items()]


# The mesh entries (include/ecm_mesh.h, prefix ecms_): the triangle mesh of the TSDF volume, counted and then written.
MESH_PROTOTYPES = {
    "ecms_mesh_tile": (_I, []),
    "ecms_mesh_brick": (_I, [_I]),
    "ecms_mesh_scratch_bytes": (_LL, [_I, _I, _I]),
    "ecms_mesh_count_fwd": (_I, [_P, _P, _P, _P, _LL, _I, _I, _I, _F, _P]),
    "ecms_mesh_emit_fwd": (_I, [_P] * 8 + [_LL, _LL, _LL, _I, _I, _I, _F, _P]),
}

MESH_TABLES = {
    "ecm_mesh.h": (MESH_PROTOTYPES, "ecms_"),
}

# tests/test_disp_volume_cpu.py pins LATER_REGISTRIES == (VOLUME_TABLES,) and the row count of _all_tables(), so a seventh header
# can be a row of neither without an edit of that file.  One more tuple of registries of the same form: load() and
# missing_symbols() walk _all_tables() and then these, so call() and query() serve them alike, and the new header's own test file
# holds it to the same census.
NEWER_REGISTRIES = (MESH_TABLES,)


def _every_table():
    return _all_tables() + [row for registry in NEWER_REGISTRIES for table, _ in registry.values() for row in table.items()]


# The colour entries (include/ecm_color.h, prefix ecmc_): attribute planes in the TSDF volume, integrated, raycast and sampled.
COLOR_PROTOTYPES = {
    "ecmc_max_attributes": (_I, []),
    "ecmc_integrate_fwd": (_I, [_P] * 11 + [_I] * 8 + [_F] * 4 + [_P]),
    "ecmc_raycast_fwd": (_I, [_P] * 6 + [_I, _P, _P, _P] + [_I] * 7 + [_F, _F, _F, _I, _P]),
    "ecmc_sample_fwd": (_I, [_P] * 5 + [_LL, _I, _I, _I, _I, _P]),
}

COLOR_TABLES = {
    "ecm_color.h": (COLOR_PROTOTYPES, "ecmc_"),
}

# tests/test_volume_mesh_cpu.py pins NEWER_REGISTRIES == (MESH_TABLES,) and the row count of _every_table(), so an eighth header can
# be a row of neither without an edit of that file.  One more tuple of registries of the same form: load() and missing_symbols()
# walk _every_table() and then these, so call() and query() serve them alike, and the new header's own test file holds it to the
# same census.
NEWEST_REGISTRIES = (COLOR_TABLES,)


def _each_table():
    return _every_table() + [row for registry in NEWEST_REGISTRIES for table, _ in registry.values() for row in table.items()]


# The augmentation entries (include/ecm_augment.h, prefix ecma_): the KITTI training transform in the frame decode, and its colour
# jitter on resident uint8 images.
AUGMENT_PROTOTYPES = {
    "ecma_jitter_tile": (_I, []),
    "ecma_jitter_scratch_bytes": (_LL, [_I, _I, _I]),
    "ecma_color_jitter_fwd": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _LL, _P]),
    "ecma_frame_prep_jitter_fwd": (_I, [_P, _P, _I] + [_P] * 4 + [_I, _I, _I, _P, _P, _I, _I] + [_P] * 7 + [_LL, _P]),
}

AUGMENT_TABLES = {
    "ecm_augment.h": (AUGMENT_PROTOTYPES, "ecma_"),
}

# tests/test_volume_color_cpu.py pins NEWEST_REGISTRIES == (COLOR_TABLES,) and the row count of _each_table(), so a ninth header can
# be a row of neither without an edit of that file.  One more tuple of registries of the same form: load() and missing_symbols()
# walk _each_table() and then these, so call() and query() serve them alike, and the new header's own test file holds it to the
# same census.
LATEST_REGISTRIES = (AUGMENT_TABLES,)


def _whole_table():
    return _each_table() + [row for registry in LATEST_REGISTRIES for table, _ in registry.values() for row in table.items()]


_lib = None


def load():
    """Load libecm_hip.so once; raise loudly if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C explicit-context-mapping-for-stereo-matching_amd/csrc`). There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _whole_table():
            fn = getattr(lib, name, None)
            if fn is None:
                continue            # reported by missing_symbols()/tests; calling it raises below
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def missing_symbols():
    lib = load()
    return [n for n, _ in _whole_table() if not hasattr(lib, n)]


# Optional per-launch timing (bench.py's roofline leg): name -> list of (start_event, end_event, int_args).
# Events are recorded on torch's current stream, which is the stream every kernel is launched on.
_timers = {}
_time_all = False


def enable_timer(name: str):
    _timers[name] = []


def enable_all_timers():
    """Time EVERY int-returning entry point from now on (bench.py's per-family step breakdown)."""
    global _time_all
    _time_all = True


def disable_timers():
    global _time_all
    out = dict(_timers)
    _timers.clear()
    _time_all = False
    return out


class _Args(tuple):
    """The integer arguments of a timed launch (what bench.py indexes); `.longs` holds the 64-bit ones (sizes) beside them,
    `.ptrs` one flag per pointer argument (False = NULL: an optional operand that was not passed)."""
    longs = ()
    ptrs = ()


def call(name: str, *args):
    """Call an int-returning entry point and raise RuntimeError on a non-zero code."""
    lib = load()
    fn = getattr(lib, name, None)
    if fn is None:
        raise RuntimeError(f"libecm_hip.so does not export {name}")
    rec = _timers.get(name)
    if rec is None and _time_all:
        rec = _timers[name] = []
    if rec is not None:
        import torch
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        rc = fn(*args)
        e.record()
        ints = _Args(a for a in args if isinstance(a, int))
        ints.longs = tuple(a.value for a in args if isinstance(a, C.c_longlong))
        ints.ptrs = tuple(a is not None and bool(a.value) for a in args if a is None or isinstance(a, C.c_void_p))   # which optional operands were passed
        rec.append((s, e, ints))
    else:
        rc = fn(*args)
    if rc != 0:
        msg = lib.ecm_error_string(rc)
        raise RuntimeError(f"{name} failed ({rc}): {msg.decode() if msg else '?'}")


def query(name: str, *args):
    """Call a value-returning entry point (sizes)."""
    return getattr(load(), name)(*args)
