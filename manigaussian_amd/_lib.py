"""ctypes binding of libmgsplat.so (C ABI declared in include/mgsplat.h).

There is no CPU fallback and no other backend: if the HIP library is missing or stale this module
raises, loudly, at import of the ops (build it with `python -c "import __graft_entry__ as g; g.build()"`
or `make -C manigaussian_amd/csrc`).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmgsplat.so")
ABI_VERSION = 17

c_fp = ctypes.c_void_p  # device pointers travel as integers (tensor.data_ptr())
c_i32 = ctypes.c_int32
c_sz = ctypes.c_size_t

# error codes (include/mgsplat.h)
MGS_OK, MGS_ERR_INVALID_ARG, MGS_ERR_HIP, MGS_ERR_WORKSPACE, MGS_ERR_NON_RGB = 0, -1, -2, -3, -4
MGS_NEED_CAPACITY = 1
MGS_PENDING = 2
MGS_RETRY_TABLE_INIT = 3  # mgs_forward_result: the preprocess's table hand-shake gave up; re-run with table_init = 1

SUPPORTED_F = (3, 4, 8, 16, 32, 64)


class MgsOptions(ctypes.Structure):
    _fields_ = [("set", c_i32), ("tight_bins", c_i32), ("fast_exp", c_i32), ("exact_cull", c_i32), ("bin_mode", c_i32),
                ("seg", c_i32), ("gm_waves", c_i32), ("dbg", c_i32), ("table_init", c_i32)]


class MgsRasterArgs(ctypes.Structure):
    _fields_ = [
        ("P", c_i32), ("D", c_i32), ("M", c_i32), ("F", c_i32), ("W", c_i32), ("H", c_i32),
        ("tanfovx", ctypes.c_float), ("tanfovy", ctypes.c_float), ("scale_modifier", ctypes.c_float),
        ("prefiltered", c_i32), ("debug", c_i32), ("include_feature", c_i32),
        ("background", c_fp), ("means3D", c_fp), ("shs", c_fp), ("colors_precomp", c_fp),
        ("language_feature", c_fp), ("opacities", c_fp), ("scales", c_fp), ("rotations", c_fp),
        ("cov3D_precomp", c_fp), ("viewmatrix", c_fp), ("projmatrix", c_fp), ("campos", c_fp),
        ("geom", c_fp), ("geom_bytes", c_sz), ("binning", c_fp), ("binning_bytes", c_sz),
        ("img", c_fp), ("img_bytes", c_sz),
        ("bwd_accum", c_fp), ("bwd_accum_bytes", c_sz), ("accum_prezeroed", c_i32),
        ("binning_capacity", c_i32), ("chunk_pool", c_i32), ("status_tag", ctypes.c_uint32), ("async_forward", c_i32),
        ("opt", MgsOptions),
    ]


class MgsView(ctypes.Structure):
    _fields_ = [("tanfovx", ctypes.c_float), ("tanfovy", ctypes.c_float), ("viewmatrix", c_fp), ("projmatrix", c_fp),
                ("campos", c_fp)]


class MgsWorkspaceRegion(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 24), ("workspace", c_i32), ("kind", c_i32), ("alias", c_i32), ("pad_", c_i32),
                ("offset", c_sz), ("bytes", c_sz)]


REGION_FLOAT, REGION_INDEX = 0, 1                       # MGS_REGION_*
WORKSPACE_NAMES = ("geom", "img", "binning")            # MGS_WORKSPACE_*


class MgsAttentionArgs(ctypes.Structure):
    _fields_ = [("B", c_i32), ("H", c_i32), ("Nq", c_i32), ("Nk", c_i32), ("D", c_i32), ("dropout_p", ctypes.c_float),
                ("q", c_fp), ("k", c_fp), ("v", c_fp), ("mask", c_fp), ("rng_state", c_fp)] + \
               [(n, ctypes.c_int64) for n in ("q_stride_b", "q_stride_n", "k_stride_b", "k_stride_n", "v_stride_b", "v_stride_n",
                                              "out_stride_b", "out_stride_n", "dout_stride_b", "dout_stride_n", "dq_stride_b",
                                              "dq_stride_n", "dkv_stride_b", "dkv_stride_n", "mask_stride_b")]


VOLUME_MAX_SOURCES = 4


class MgsVolumeArgs(ctypes.Structure):
    _fields_ = [("B", c_i32), ("D", c_i32), ("H", c_i32), ("W", c_i32), ("scale", c_i32), ("pad", c_i32), ("nsrc", c_i32),
                ("C", c_i32 * VOLUME_MAX_SOURCES), ("src", c_fp * VOLUME_MAX_SOURCES),
                ("stride_b", ctypes.c_int64 * VOLUME_MAX_SOURCES), ("stride_c", ctypes.c_int64 * VOLUME_MAX_SOURCES)]


SE3_MAX_SOURCES, SE3_MAX_BATCH, SE3_MAX_ATTEMPTS = 8, 4096, 32  # MGS_SE3_MAX_*


class MgsSe3Args(ctypes.Structure):
    _fields_ = [(n, c_i32) for n in ("B", "attempts", "retry", "layer", "voxel_size", "bounds_rows", "rot_bins", "trans_f64",
                                     "action_i64")] + \
               [("rot_steps", c_i32 * 3), ("rot_step_rad", ctypes.c_float), ("n_sources", c_i32), ("n_poses", c_i32),
                ("pad_", c_i32), ("rot_resolution", ctypes.c_double), ("trans_aug_range", ctypes.c_double * 3),
                ("gripper_pose", c_fp), ("action_trans", c_fp), ("action_rot_grip", c_fp), ("bounds", c_fp), ("rng_state", c_fp),
                ("draws", c_fp), ("src", c_fp * SE3_MAX_SOURCES), ("dst", c_fp * SE3_MAX_SOURCES),
                ("n_points", ctypes.c_int64 * SE3_MAX_SOURCES), ("stride_b", ctypes.c_int64 * SE3_MAX_SOURCES),
                ("stride_c", ctypes.c_int64 * SE3_MAX_SOURCES), ("pose_in", c_fp * SE3_MAX_SOURCES),
                ("pose_out", c_fp * SE3_MAX_SOURCES)]


MAX_VIEWS = 16  # views of a batch; also the most Gaussian sets of a set batch
c_i64 = ctypes.c_int64


class MgsPlanShape(ctypes.Structure):
    _fields_ = [(n, c_i32) for n in ("P", "M", "F", "W", "H", "V", "S", "colors_precomp")]


class MgsArenaPlan(ctypes.Structure):
    _fields_ = [("geom_bytes", c_sz), ("img_bytes", c_sz), ("worst_bytes", c_sz), ("worst_capacity", c_i64),
                ("worst_pool", c_i32), ("worst_fits", c_i32)]


class MgsGradientPlan(ctypes.Structure):
    _fields_ = [(n, c_i64) for n in ("scratch", "colors", "feature", "means3D", "opacity", "sh", "scales", "rotations", "cov3D",
                                     "means2D", "pad", "total")] + [("accum_bytes", c_sz)]


SIZE_HEADROOM, SIZE_COUNT = 0, 1  # mgs_plan_capacity: marks x head-room | a mark or a reported count (R < 0: none known)


# ---- the report ledger (include/mgsplat.h "the report ledger") ----
class MgsLedgerConfig(ctypes.Structure):
    _fields_ = [("mode", c_i32), ("overflow_policy", c_i32), ("head_instances", ctypes.c_double),
                ("head_chunks", ctypes.c_double), ("safe_bytes", c_i64)]


class MgsMarkKey(ctypes.Structure):
    _fields_ = [(n, c_i32) for n in ("V", "S", "P", "W", "H", "F", "tight_bins")]


class MgsReport(ctypes.Structure):
    _fields_ = [(n, c_i32) for n in ("rc", "num_rendered", "chunks_used", "ref_rendered")]


class MgsLedgerOut(ctypes.Structure):
    _fields_ = [("error", ctypes.c_char_p), ("n_warnings", c_i32), ("warnings", ctypes.POINTER(ctypes.c_char_p))]


LEDGER_SLOT_WORDS = 4
TICKET_RECOVERABLE, TICKET_CAPTURED = 1, 2
LEDGER_SYNC_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p)  # mgs_ledger_drain's sync_fn (None: the library synchronises)

_EXPORTS = {
    # name: (restype, argtypes)
    "mgs_abi_version": (ctypes.c_int, []),
    "mgs_last_error": (ctypes.c_char_p, []),
    "mgs_build_id": (ctypes.c_char_p, []),
    "mgs_options_default": (None, [ctypes.POINTER(MgsOptions)]),
    "mgs_set_option": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]),
    "mgs_get_option": (ctypes.c_int, [ctypes.c_char_p]),
    "mgs_geom_bytes": (c_sz, [ctypes.c_int] * 4),
    "mgs_img_bytes": (c_sz, [ctypes.c_int, ctypes.c_int]),
    "mgs_binning_bytes": (c_sz, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "mgs_binning_bytes2": (c_sz, [ctypes.c_int] * 5),
    "mgs_binning_direct_extra": (c_sz, [ctypes.c_int] * 4),
    "mgs_chunk_pool_max": (ctypes.c_int, [ctypes.c_int] * 3),
    "mgs_plan_arena": (ctypes.c_int, [ctypes.POINTER(MgsPlanShape), c_i64, ctypes.POINTER(MgsArenaPlan)]),
    "mgs_plan_binning_bytes": (c_sz, [ctypes.POINTER(MgsPlanShape), c_i64, c_i64, ctypes.c_int]),
    "mgs_plan_capacity": (ctypes.c_int, [ctypes.POINTER(MgsPlanShape), ctypes.c_int, c_i64, c_i64, ctypes.c_double,
                                         ctypes.c_double, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    "mgs_plan_options": (ctypes.c_int, [ctypes.POINTER(MgsPlanShape), c_i64, ctypes.POINTER(MgsOptions)]),
    "mgs_plan_gradients": (ctypes.c_int, [ctypes.POINTER(MgsPlanShape), ctypes.POINTER(MgsGradientPlan)]),
    "mgs_ledger_set_config": (None, [ctypes.POINTER(MgsLedgerConfig)]),
    "mgs_ledger_get_config": (None, [ctypes.POINTER(MgsLedgerConfig)]),
    "mgs_ledger_ring": (c_fp, [ctypes.c_int, c_fp, ctypes.c_int]),
    "mgs_ledger_ring_slots": (ctypes.c_int, [ctypes.c_int]),
    "mgs_ledger_take_slot": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(c_fp), ctypes.POINTER(ctypes.c_uint32)]),
    "mgs_marks_get": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(MgsMarkKey), ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    "mgs_marks_set": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(MgsMarkKey), c_i64, c_i64]),
    "mgs_marks_erase": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(MgsMarkKey)]),
    "mgs_marks_keys": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(MgsMarkKey), ctypes.c_int]),
    "mgs_marks_learn": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(MgsMarkKey), c_i64, c_i64, ctypes.c_int]),
    "mgs_marks_guess": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(MgsMarkKey), ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    "mgs_ledger_hold": (ctypes.c_int, [ctypes.c_int, c_i64, c_i64]),
    "mgs_ledger_unhold": (None, [ctypes.c_int, c_i64]),
    "mgs_ledger_held": (c_i64, [ctypes.c_int]),
    "mgs_ledger_add": (c_fp, [ctypes.c_int, ctypes.POINTER(MgsRasterArgs), c_i32, c_fp, ctypes.POINTER(MgsMarkKey), ctypes.c_int]),
    "mgs_ledger_poll": (ctypes.c_int, [c_fp, ctypes.POINTER(MgsReport)]),
    "mgs_ledger_backward_enqueued": (None, [c_fp]),
    "mgs_ledger_superseded": (None, [c_fp]),
    "mgs_ledger_release": (None, [c_fp]),
    "mgs_ledger_outstanding": (ctypes.c_int, [ctypes.c_int]),
    "mgs_ledger_drain": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, LEDGER_SYNC_FN, c_fp, ctypes.POINTER(MgsLedgerOut)]),
    "mgs_ledger_check_captured": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(MgsLedgerOut)]),
    "mgs_ledger_lost_step_message": (ctypes.c_char_p, [ctypes.c_int]),
    "mgs_forward_result": (ctypes.c_int, [ctypes.POINTER(MgsRasterArgs), c_fp, ctypes.POINTER(c_i32),
                                          ctypes.POINTER(c_i32), ctypes.POINTER(c_i32)]),
    "mgs_forward_result_views": (ctypes.c_int, [ctypes.POINTER(MgsRasterArgs), c_i32, c_fp, ctypes.POINTER(c_i32),
                                                ctypes.POINTER(c_i32), ctypes.POINTER(c_i32)]),
    "mgs_views_binning_bytes2": (c_sz, [ctypes.c_int] * 6),
    "mgs_views_chunk_pool_max": (ctypes.c_int, [ctypes.c_int] * 4),
    "mgs_calibration_kernel": (ctypes.c_int, [ctypes.c_int, c_fp, c_fp]),
    "mgs_backward_scratch_bytes": (c_sz, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "mgs_rasterize_forward_preprocess": (ctypes.c_int, [ctypes.POINTER(MgsRasterArgs), c_fp,
                                                        ctypes.POINTER(c_i32), c_fp]),
    "mgs_rasterize_forward_render": (ctypes.c_int, [ctypes.POINTER(MgsRasterArgs), c_i32, c_fp, c_fp, c_fp, c_fp]),
    "mgs_rasterize_forward": (ctypes.c_int, [ctypes.POINTER(MgsRasterArgs), c_fp, c_fp, c_fp, ctypes.POINTER(c_i32),
                                             c_fp, c_fp]),
    "mgs_rasterize_backward": (ctypes.c_int, [ctypes.POINTER(MgsRasterArgs), c_i32, c_fp] + [c_fp] * 12 +
                               [c_fp, c_sz, c_fp]),
    "mgs_views_geom_bytes": (c_sz, [ctypes.c_int] * 5),
    "mgs_views_img_bytes": (c_sz, [ctypes.c_int] * 3),
    "mgs_views_binning_bytes": (c_sz, [ctypes.c_int] * 5),
    "mgs_views_backward_scratch_bytes": (c_sz, [ctypes.c_int] * 4),
    "mgs_rasterize_forward_views": (ctypes.c_int, [ctypes.POINTER(MgsRasterArgs), c_i32, ctypes.POINTER(MgsView), c_fp,
                                                   c_fp, c_fp, ctypes.POINTER(c_i32), c_fp, c_fp]),
    "mgs_rasterize_backward_views": (ctypes.c_int, [ctypes.POINTER(MgsRasterArgs), c_i32, ctypes.POINTER(MgsView), c_i32,
                                                    c_fp] + [c_fp] * 12 + [c_fp, c_sz, c_fp]),
    "mgs_sets_backward_scratch_bytes": (c_sz, [ctypes.c_int] * 5),
    "mgs_rasterize_forward_sets": (ctypes.c_int, [ctypes.POINTER(MgsRasterArgs), c_i32, ctypes.POINTER(MgsView), c_i32,
                                                  ctypes.POINTER(c_i32), c_fp, c_fp, c_fp, ctypes.POINTER(c_i32), c_fp, c_fp]),
    "mgs_rasterize_backward_sets": (ctypes.c_int, [ctypes.POINTER(MgsRasterArgs), c_i32, ctypes.POINTER(MgsView), c_i32,
                                                   ctypes.POINTER(c_i32), c_i32, c_fp] + [c_fp] * 12 + [c_fp, c_sz, c_fp]),
    "mgs_mark_visible": (ctypes.c_int, [ctypes.c_int, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "mgs_deform_assemble_forward": (ctypes.c_int, [ctypes.c_int] * 4 + [c_fp] * 10 + [c_fp]),
    "mgs_deform_assemble_backward": (ctypes.c_int, [ctypes.c_int] * 5 + [c_fp] * 3 + [c_fp]),
    "mgs_deform_apply_forward": (ctypes.c_int, [ctypes.c_int] + [c_fp] * 5 + [c_fp]),
    "mgs_deform_apply_backward": (ctypes.c_int, [ctypes.c_int] + [c_fp] * 5 + [c_fp]),
    "mgs_mlp_relu_bias": (ctypes.c_int, [ctypes.c_int] * 2 + [c_fp] * 4 + [c_fp]),
    "mgs_mlp_relu_backward": (ctypes.c_int, [ctypes.c_int] * 2 + [c_fp] * 5 + [c_fp]),
    "mgs_regress_epilogue_forward": (ctypes.c_int, [ctypes.c_int] + [c_fp] * 9 + [c_fp]),
    "mgs_regress_epilogue_backward": (ctypes.c_int, [ctypes.c_int] + [c_fp] * 9 + [c_fp]),
    "mgs_voxel_sample_pe_forward": (ctypes.c_int, [ctypes.c_int] * 6 + [ctypes.c_float, ctypes.POINTER(ctypes.c_float)] +
                                    [c_fp] * 3 + [c_fp]),
    "mgs_voxel_sample_backward": (ctypes.c_int, [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_float)] + [c_fp] * 2 +
                                  [ctypes.c_int, c_fp, c_fp]),
    "mgs_novel_calib": (ctypes.c_int, [ctypes.c_int, c_fp, c_fp, ctypes.c_int, ctypes.c_int] + [ctypes.c_float] * 6 +
                        [c_fp] * 5 + [c_fp, c_fp]),
    "mgs_novel_calib_host": (ctypes.c_int, [ctypes.c_int, c_fp, c_fp, ctypes.c_int, ctypes.c_int] + [ctypes.c_float] * 6 +
                             [c_fp] * 5),
    "mgs_render_loss_workspace_bytes": (c_sz, [ctypes.c_int] * 3),
    "mgs_render_loss_forward": (ctypes.c_int, [ctypes.c_int] * 4 + [c_fp, c_fp, ctypes.POINTER(ctypes.c_int64), c_fp, c_fp,
                                               ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.POINTER(ctypes.c_float),
                                               c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_sz, c_fp]),
    "mgs_render_loss_backward": (ctypes.c_int, [ctypes.c_int] * 4 + [c_fp] * 5 + [c_fp]),
    "mgs_photometric_workspace_bytes": (c_sz, [ctypes.c_int] * 4),
    "mgs_photometric_forward": (ctypes.c_int, [ctypes.c_int] * 4 + [c_fp, c_fp, ctypes.POINTER(ctypes.c_int64),
                                               ctypes.POINTER(ctypes.c_float), c_fp, c_fp, c_fp, c_fp, c_fp, c_sz, c_fp]),
    "mgs_photometric_backward": (ctypes.c_int, [ctypes.c_int] * 4 + [c_fp, ctypes.c_int, c_fp, c_fp, c_fp]),
    "mgs_lamb_chunk_elems": (ctypes.c_int, []),
    "mgs_lamb_workspace_bytes": (c_sz, [ctypes.c_int64]),
    "mgs_lamb_step": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp,
                                     ctypes.c_float, ctypes.c_int, c_fp, c_sz, c_fp]),
    "mgs_voxelize_workspace_bytes": (c_sz, [ctypes.c_int, ctypes.c_int64, ctypes.c_int]),
    "mgs_voxelize_forward": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64] + [ctypes.c_int] * 3 + [c_fp] * 5 + [c_sz, c_fp]),
    "mgs_voxelize_forward_images": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64] + [ctypes.c_int] * 3 +
                                    [ctypes.POINTER(c_fp)] * 2 + [c_fp] * 3 + [c_sz, c_fp]),
    "mgs_attention_workspace_bytes": (c_sz, [ctypes.c_int] * 4),
    "mgs_attention_forward": (ctypes.c_int, [ctypes.POINTER(MgsAttentionArgs), c_fp, c_fp, c_fp]),
    "mgs_attention_backward": (ctypes.c_int, [ctypes.POINTER(MgsAttentionArgs)] + [c_fp] * 6 + [c_sz, c_fp]),
    "mgs_attention_dropout_mask": (ctypes.c_int, [ctypes.POINTER(MgsAttentionArgs), c_fp, c_fp]),
    "mgs_se3_workspace_bytes": (c_sz, [ctypes.c_int]),
    "mgs_se3_select": (ctypes.c_int, [ctypes.POINTER(MgsSe3Args), c_fp, c_fp, c_fp, c_fp, c_sz, c_fp]),
    "mgs_se3_apply": (ctypes.c_int, [ctypes.POINTER(MgsSe3Args), c_fp, c_sz, c_fp]),
    "mgs_se3_draws": (ctypes.c_int, [ctypes.POINTER(MgsSe3Args), c_fp, c_fp]),
    "mgs_spatial_softmax_workspace_bytes": (c_sz, [ctypes.c_int64] * 2),
    "mgs_spatial_softmax_forward": (ctypes.c_int, [ctypes.c_int64] + [ctypes.c_int] * 4 + [ctypes.c_float, c_fp, c_fp, ctypes.c_int64,
                                                   c_fp, ctypes.c_int64, c_fp, c_fp, c_sz, ctypes.c_int, c_fp]),
    "mgs_spatial_softmax_backward": (ctypes.c_int, [ctypes.c_int64] + [ctypes.c_int] * 4 + [ctypes.c_float, c_fp, c_fp, c_fp,
                                                    ctypes.c_int64, c_fp, ctypes.c_int64, c_fp, ctypes.c_int, c_fp]),
    "mgs_volume_workspace_bytes": (c_sz, [ctypes.POINTER(MgsVolumeArgs)]),
    "mgs_volume_resample_pad_forward": (ctypes.c_int, [ctypes.POINTER(MgsVolumeArgs), c_fp, c_fp]),
    "mgs_volume_resample_pad_backward": (ctypes.c_int, [ctypes.POINTER(MgsVolumeArgs), c_fp, ctypes.POINTER(c_fp), c_fp, c_sz, c_fp]),
    "mgs_feedforward_workspace_bytes": (c_sz, [ctypes.c_int64] * 2),
    "mgs_layernorm_forward": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, c_fp, ctypes.c_int64, c_fp, c_fp, ctypes.c_float,
                                             c_fp, c_fp, c_fp]),
    "mgs_layernorm_backward": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, c_fp, ctypes.c_int64, c_fp, c_fp, c_fp, ctypes.c_int64,
                                              c_fp, c_fp, c_fp, c_fp, c_sz, ctypes.c_int, c_fp]),
    "mgs_bias_geglu_forward": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, c_fp, ctypes.c_int64, c_fp, c_fp, c_fp]),
    "mgs_bias_geglu_backward": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, c_fp, ctypes.c_int64, c_fp, c_fp, ctypes.c_int64,
                                               c_fp, c_fp, c_fp, c_sz, ctypes.c_int, c_fp]),
    "mgs_abn_workspace_bytes": (c_sz, [ctypes.c_int64, ctypes.c_int, ctypes.c_int64]),
    "mgs_abn_forward": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int64] + [c_fp] * 7 + [ctypes.c_int] +
                        [ctypes.c_float] * 3 + [c_fp, c_fp, c_fp, c_sz, ctypes.c_int, c_fp]),
    "mgs_abn_backward": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int64] + [c_fp] * 5 + [ctypes.c_float] +
                         [c_fp] * 4 + [c_sz, ctypes.c_int, c_fp]),
    "mgs_conv3d_workspace_bytes": (c_sz, [ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_int64] * 3 + [ctypes.c_int]),
    "mgs_conv3d_forward": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_int64] * 3 + [ctypes.c_int] +
                           [c_fp] * 4),
    "mgs_conv3d_backward_data": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_int64] * 3 +
                                 [ctypes.c_int] + [c_fp] * 4),
    "mgs_conv3d_backward_weight": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_int64] * 3 +
                                   [ctypes.c_int] + [c_fp] * 4 + [c_sz, ctypes.c_int, c_fp]),
    "mgs_pointwise_workspace_bytes": (c_sz, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int64]),
    "mgs_pointwise_forward": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int64] + [c_fp] * 5),
    "mgs_pointwise_backward": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int64] + [c_fp] * 7 +
                               [c_sz, ctypes.c_int, c_fp]),
    "mgs_pointwise_wide_workspace_bytes": (c_sz, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int64]),
    "mgs_pointwise_wide_forward": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int64] + [c_fp] * 5),
    "mgs_pointwise_wide_backward": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int64] + [c_fp] * 7 +
                                    [c_sz, ctypes.c_int, c_fp]),
    "mgs_narrow_conv3d_workspace_bytes": (c_sz, [ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_int64] * 3),
    "mgs_narrow_conv3d_forward": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_int64] * 3 + [ctypes.c_int] +
                                  [c_fp] * 5),
    "mgs_narrow_conv3d_backward": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_int64] * 3 +
                                   [ctypes.c_int] + [c_fp] * 7 + [c_sz, ctypes.c_int, c_fp]),
    "mgs_dense_conv3d_workspace_bytes": (c_sz, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_int64] * 3),
    "mgs_dense_conv3d_forward": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_int64] * 3 +
                                 [ctypes.c_float] + [c_fp] * 5 + [c_sz, c_fp]),
    "mgs_dense_conv3d_backward": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_int64] * 3 +
                                  [ctypes.c_float] + [c_fp] * 9 + [c_sz, ctypes.c_int, c_fp]),
    "mgs_patch_conv3d_workspace_bytes": (c_sz, [ctypes.c_int64] + [ctypes.c_int] * 4 + [ctypes.c_int64] * 3),
    "mgs_patch_conv3d_forward": (ctypes.c_int, [ctypes.c_int64] + [ctypes.c_int] * 4 + [ctypes.c_int64] * 3 +
                                 [ctypes.c_int, ctypes.c_float] + [c_fp] * 5 + [c_sz, c_fp]),
    "mgs_patch_conv3d_backward": (ctypes.c_int, [ctypes.c_int64] + [ctypes.c_int] * 4 + [ctypes.c_int64] * 3 +
                                  [ctypes.c_int, ctypes.c_float] + [c_fp] * 8 + [c_sz, ctypes.c_int, c_fp]),
    "mgs_forward_stats": (ctypes.c_int, [ctypes.POINTER(MgsRasterArgs), c_i32, ctypes.POINTER(ctypes.c_int64),
                                         ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), c_fp]),
    "mgs_debug_geom_layout": (ctypes.c_int, [ctypes.c_int] * 4 + [ctypes.POINTER(c_sz)] * 4),
    "mgs_debug_binning_layout": (ctypes.c_int, [ctypes.POINTER(MgsRasterArgs), c_i32] + [ctypes.POINTER(c_sz)] * 3 +
                                 [ctypes.POINTER(c_i32)]),
    "mgs_debug_direct_keys": (ctypes.c_int, [ctypes.POINTER(MgsRasterArgs), c_i32, ctypes.POINTER(c_sz), ctypes.POINTER(c_i32)]),
    "mgs_debug_workspace_regions": (ctypes.c_int, [ctypes.POINTER(MgsRasterArgs), c_i32, ctypes.POINTER(MgsWorkspaceRegion), c_i32,
                                                   ctypes.POINTER(c_i32)]),
    "mgs_debug_read_trace": (ctypes.c_int, [ctypes.c_void_p, c_sz]),
    "mgs_debug_read_trace_bwd": (ctypes.c_int, [ctypes.c_void_p, c_sz]),
    "mgs_debug_read_trace_bin": (ctypes.c_int, [ctypes.c_void_p, c_sz]),
    "mgs_selftest": (ctypes.c_int, [c_fp]),
    "mgs_profile_num_stages": (ctypes.c_int, []),
    "mgs_profile_stage_name": (ctypes.c_char_p, [ctypes.c_int]),
    "mgs_profile_read": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_i32), ctypes.c_int]),
}

_lib = None


def exported_symbols():
    """Every entry point include/mgsplat.h declares."""
    return sorted(_EXPORTS)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: the HIP library is not built. There is no fallback path; run "
                "`make -C manigaussian_amd/csrc` (hipcc, gfx950) or __graft_entry__.build().")
        L = ctypes.CDLL(LIB_PATH)
        for name, (rt, at) in _EXPORTS.items():
            fn = getattr(L, name)  # AttributeError if the .so is stale
            fn.restype, fn.argtypes = rt, at
        v = L.mgs_abi_version()
        if v != ABI_VERSION:
            raise ImportError(f"libmgsplat ABI version {v} != expected {ABI_VERSION}; rebuild")
        _lib = L
    return _lib


def build_id() -> str:
    """Hash of the sources libmgsplat.so was compiled from (baked in at build time)."""
    return lib().mgs_build_id().decode()


def last_error() -> str:
    return lib().mgs_last_error().decode("utf-8", "replace")


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {last_error()} (code {rc})")


# Per-call tuning switches (MgsOptions): the C ABI has no process-wide option state; this dict is merely the DEFAULT the
# Python shim copies into every call's MgsRasterArgs.opt (a forward's values travel to its backward in the autograd ctx).
DEFAULT_OPTIONS = dict(tight_bins=1, fast_exp=0, exact_cull=1, bin_mode=2, seg=2048, gm_waves=12, dbg=0, table_init=0)
OPTIONS_VERSION = [0]  # bumped by set_option: callers that cache a filled MgsOptions key it on this


def set_option(key: str, value: int):
    """"profile": the library's one process-wide DIAGNOSTIC switch (stage timers).  Any other key: the default of the
    per-call option of that name for calls made from this process afterwards."""
    if key == "profile":
        check(lib().mgs_set_option(key.encode(), int(value)), "mgs_set_option")
    elif key in DEFAULT_OPTIONS:
        if key == "seg" and int(value) not in (512, 1024, 2048, 4096):
            raise RuntimeError("seg must be 512, 1024, 2048 or 4096")
        DEFAULT_OPTIONS[key] = int(value)
        OPTIONS_VERSION[0] += 1
        push_options()
    else:
        raise RuntimeError(f"unknown option {key}")


def push_options():
    """Hand the per-call defaults to the compiled binding (it fills MgsRasterArgs.opt itself)."""
    from . import _state
    e = _state._EXT[0]
    if e:
        o = DEFAULT_OPTIONS
        e.set_options(o["tight_bins"], o["fast_exp"], o["exact_cull"], o["bin_mode"], o["seg"], o["gm_waves"], o["dbg"],
                      o["table_init"])


def get_option(key: str) -> int:
    if key == "profile":
        return lib().mgs_get_option(key.encode())
    return DEFAULT_OPTIONS[key]


# ---- the workspace plan (include/mgsplat.h "the workspace plan"): how large, asked of the library ONCE per distinct question ----
_PLANS = {}  # (query, its arguments) -> the library's answer: a warm forward sizes itself without a call into the library


def _planned(query):
    def ask(*key):
        k = (query, key)
        v = _PLANS.get(k, _PLANS)  # (the dict itself stands for "not asked yet": None is an answer)
        if v is _PLANS:
            if len(_PLANS) > 4096:  # marks that keep growing: drop the answers keyed by counts, keep the per-shape ones
                for old in [o for o in _PLANS if o[0] in _BY_COUNT]:
                    del _PLANS[old]
                if len(_PLANS) > 2048:
                    _PLANS.clear()
            v = _PLANS[k] = query(lib(), *key)
        return v
    ask.query = query
    return ask


@_planned
def plan_arena(L, P, M, F, W, H, V, budget):
    """(geom bytes, img bytes, the worst case fits the budget, its capacity, chunk pool, binning bytes); V: 0 or a batch's views."""
    o = MgsArenaPlan()
    check(L.mgs_plan_arena(MgsPlanShape(P, M, F, W, H, V), budget, o), "mgs_plan_arena")
    return o.geom_bytes, o.img_bytes, bool(o.worst_fits), o.worst_capacity, o.worst_pool, o.worst_bytes


@_planned
def plan_binning_bytes(L, P, F, W, H, V, capacity, pool, direct_room):
    """Bytes of the binning workspace (pool 0: the worst case for the capacity); direct_room: plus the room in which the forward
    preprocess writes the tile keys itself (no bin scatter launch) where the library offers it for the shape."""
    n = L.mgs_plan_binning_bytes(MgsPlanShape(P, 0, F, W, H, V), capacity, pool, int(direct_room))
    if not n:
        raise RuntimeError(f"mgs_plan_binning_bytes: {last_error()}")
    return n


@_planned
def plan_capacity(L, how, P, V, R, chunks=0, head_instances=1.0, head_chunks=1.0):
    """(capacity, chunk pool) of a forward sized from earlier ones of its shape: SIZE_HEADROOM or SIZE_COUNT."""
    cap, pool = c_i64(), c_i64()
    check(L.mgs_plan_capacity(MgsPlanShape(P, 0, 0, 1, 1, V), how, R, chunks, head_instances, head_chunks, cap, pool),
          "mgs_plan_capacity")
    return cap.value, pool.value


@_planned
def plan_options(L, seg, bin_mode, R, W, H, V):
    """(seg, bin_mode) as the library tunes them for a shape whose forwards binned R instances, or None: as they are."""
    o = MgsOptions(seg=seg, bin_mode=bin_mode)
    check(L.mgs_plan_options(MgsPlanShape(0, 0, 0, W, H, V), R, o), "mgs_plan_options")
    return None if (o.seg, o.bin_mode) == (seg, bin_mode) else (o.seg, o.bin_mode)


@_planned
def plan_gradients(L, P, M, F, V, S, precomp):
    """(float offsets of the eleven regions of the backward's single allocation, total floats, bytes of its accumulator block)."""
    o = MgsGradientPlan()
    check(L.mgs_plan_gradients(MgsPlanShape(P, M, F, 1, 1, V, S, int(bool(precomp))), o), "mgs_plan_gradients")
    return tuple(getattr(o, n) for n, _ in MgsGradientPlan._fields_[:11]), o.total, o.accum_bytes


_BY_COUNT = {plan_binning_bytes.query, plan_capacity.query, plan_options.query}  # keyed by marks / counts beside the shape


def fill_options(a, opts=None):
    """Copy per-call options into a.opt (opts: a dict snapshot, default: DEFAULT_OPTIONS); returns the snapshot."""
    o = DEFAULT_OPTIONS if opts is None else opts
    q = a.opt
    q.set = 1
    q.tight_bins, q.fast_exp, q.exact_cull, q.bin_mode = o["tight_bins"], o["fast_exp"], o["exact_cull"], o["bin_mode"]
    q.seg, q.gm_waves, q.dbg, q.table_init = o["seg"], o["gm_waves"], o["dbg"], o["table_init"]
    return o if opts is not None else dict(o)


def workspace_regions(a, V=0):
    """mgs_debug_workspace_regions: [(workspace name, region name, byte offset, bytes, kind, alias)] of a forward's three
    workspaces in carving order (a: its MgsRasterArgs; host code only, no device needed)."""
    L = lib()
    out, n = (MgsWorkspaceRegion * 32)(), c_i32(0)
    check(L.mgs_debug_workspace_regions(ctypes.byref(a), V, out, 32, ctypes.byref(n)), "mgs_debug_workspace_regions")
    return [(WORKSPACE_NAMES[r.workspace], r.name.decode(), int(r.offset), int(r.bytes), int(r.kind), int(r.alias))
            for r in out[:n.value]]


def profile_read(reset: bool = True):
    """{stage name: (total ms, launches)} from the library's hipEvent stage timers."""
    L = lib()
    n = L.mgs_profile_num_stages()
    ms = (ctypes.c_double * n)()
    cnt = (c_i32 * n)()
    check(L.mgs_profile_read(ms, cnt, int(reset)), "mgs_profile_read")
    return {L.mgs_profile_stage_name(i).decode(): (ms[i], cnt[i]) for i in range(n)}
