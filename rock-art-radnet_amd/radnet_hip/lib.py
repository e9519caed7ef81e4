"""ctypes binding of libradnet_hip.so (C ABI declared in include/radnet_hip.h).

Thin by design: every function takes raw device pointers (torch-ROCm `tensor.data_ptr()`), sizes and
a context; no torch types cross the boundary.  There is NO CPU fallback: if the shared library is
missing or no gfx950 device is present, loading / context creation raises.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RADNET_HIP_LIBRARY", os.path.join(_HERE, "libradnet_hip.so"))    # override: A/B builds, diag twin
HEADER_PATH = os.path.abspath(os.path.join(_HERE, "..", "..", "include", "radnet_hip.h"))

c_float_p = C.c_void_p      # device pointers travel as integers
_lib = None


class RadnetError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    """Mirror of `radnet_conv_desc` (include/radnet_hip.h)."""
    _fields_ = [
        ("x", C.c_void_p), ("w", C.c_void_p), ("y", C.c_void_p),
        ("scale", C.c_void_p), ("shift", C.c_void_p), ("addend", C.c_void_p),
        ("nb", C.c_int32), ("h", C.c_int32), ("w_", C.c_int32), ("c", C.c_int32),
        ("oh", C.c_int32), ("ow", C.c_int32),
        ("kh", C.c_int32), ("kw", C.c_int32), ("stride", C.c_int32), ("pad_t", C.c_int32), ("pad_l", C.c_int32),
        ("n", C.c_int32),
        ("ldw", C.c_int32), ("ldy", C.c_int32), ("ld_add", C.c_int32),
        ("act", C.c_int32), ("act_cols", C.c_int32),
        ("dy", C.c_void_p), ("gscale", C.c_void_p), ("dx", C.c_void_p), ("dx_add", C.c_void_p), ("dx_mask", C.c_void_p),
        ("dw", C.c_void_p),
        ("ld_dy", C.c_int32), ("ld_dx", C.c_int32), ("ld_dx_add", C.c_int32), ("ld_dx_mask", C.c_int32),
        ("dw_accumulate", C.c_int32),
        ("db", C.c_void_p),
    ]


# ---- layer programs and composed entry points (include/radnet_hip.h, csrc/program.hip) --------------------------------
OP_CONV_FWD, OP_CONV_DGRAD, OP_CONV_WGRAD, OP_MAXPOOL, OP_COLSUM, OP_WINO, OP_WINO_REUSE, OP_WINO_WGRAD, OP_SCATTER, OP_FILL0, \
    OP_RELU_MASK, OP_ROI_BWD, OP_CONV_BWD, OP_CHAIN, OP_CONV_FWD_PAIR, OP_CONV_BNECK = range(1, 17)
OP_CONV_FWD_BF16 = 17
OP_CONV_DGRAD_BF16, OP_CONV_WGRAD_BF16 = 18, 19
OP_NOP = 0


class Op(C.Structure):
    """Mirror of `radnet_op`: one launch of a layer program."""
    _fields_ = [("kind", C.c_int32), ("i", C.c_int32 * 11), ("p", C.c_void_p * 8), ("conv", ConvDesc)]


class HeadDesc(C.Structure):
    """Mirror of `radnet_head_desc`."""
    _fields_ = [("fmap", C.c_void_p), ("fh", C.c_int32), ("fw", C.c_int32), ("fc", C.c_int32),
                ("rois", C.c_void_p), ("n_rois", C.c_int32), ("pool", C.c_int32), ("pooled", C.c_void_p),
                ("fwd_ops", C.POINTER(Op)), ("n_fwd", C.c_int32),
                ("y5", C.c_void_p), ("hw", C.c_int32), ("feat_c", C.c_int32), ("feat", C.c_void_p),
                ("dense_w", C.c_void_p), ("dense_ld", C.c_int32), ("dense_b", C.c_void_p), ("nc", C.c_int32), ("nreg", C.c_int32),
                ("p_cls", C.c_void_p), ("p_regr", C.c_void_p), ("tail_scratch", C.c_void_p)]


class TileDesc(C.Structure):
    """Mirror of `radnet_tile_desc`."""
    _fields_ = [("img_u8", C.c_void_p), ("h", C.c_int32), ("w", C.c_int32), ("x", C.c_void_p),
                ("base_ops", C.POINTER(Op)), ("n_base", C.c_int32),
                ("rpn_ops", C.POINTER(Op)), ("n_rpn", C.c_int32),
                ("pred", C.c_void_p), ("ld_pred", C.c_int32), ("fh", C.c_int32), ("fw", C.c_int32), ("a", C.c_int32),
                ("anchor_wh_host", C.POINTER(C.c_double)), ("std_scaling", C.c_double), ("overlap_thresh", C.c_double), ("max_boxes", C.c_int32),
                ("R", C.c_void_p), ("Rp", C.c_void_p), ("Rn", C.c_void_p), ("prop_ws", C.c_void_p),
                ("head", C.POINTER(HeadDesc))]


class DetectTailDesc(C.Structure):
    """Mirror of `radnet_detect_tail_desc`."""
    _fields_ = [("p_cls", C.c_void_p), ("p_regr", C.c_void_p), ("rois", C.c_void_p), ("n", C.c_void_p),
                ("rows", C.c_int32), ("nc", C.c_int32), ("k", C.c_int32), ("bg", C.c_int32),
                ("bbox_threshold", C.c_float), ("regr_std", C.c_float * 4),
                ("rpn_stride", C.c_double), ("nms_thresh", C.c_double), ("ratio", C.c_double),
                ("max_boxes", C.c_int32), ("out", C.c_void_p)]


class FinalNmsDesc(C.Structure):
    """Mirror of `radnet_final_nms_desc`."""
    _fields_ = [("boxes", C.c_void_p), ("probs", C.c_void_p), ("offsets", C.c_void_p),
                ("n_groups", C.c_int32), ("capacity", C.c_int32),
                ("obj_avg_threshold", C.c_double), ("obj_confidence_threshold", C.c_float), ("n_obj_avg", C.c_int32),
                ("out_boxes", C.c_void_p), ("out_probs", C.c_void_p), ("out_count", C.c_void_p), ("out_status", C.c_void_p),
                ("ws", C.c_void_p)]


class ScanTile(C.Structure):
    """Mirror of `radnet_scan_tile` (16 bytes; engine.SCAN_TILE is the same row as a NumPy dtype)."""
    _fields_ = [("slot", C.c_int32), ("ox", C.c_int32), ("oy", C.c_int32), ("image", C.c_int32)]


class ScanMergeDesc(C.Structure):
    """Mirror of `radnet_scan_merge_desc`."""
    _fields_ = [("pool", C.c_void_p), ("pool_words", C.c_int64), ("slot_rows", C.c_int32),
                ("tiles_host", C.c_void_p), ("tiles_dev", C.c_void_p),
                ("n_tiles", C.c_int32), ("nc", C.c_int32),
                ("obj_avg_threshold", C.c_double), ("obj_confidence_threshold", C.c_float), ("n_obj_avg", C.c_int32),
                ("nms_thresh", C.c_double), ("max_boxes", C.c_int32),
                ("out", C.c_void_p), ("ws", C.c_void_p)]


AUG_BRIGHTNESS, AUG_CONTRAST, AUG_SALT_PEPPER, AUG_GAUSSIAN, AUG_POISSON = range(5)      # RADNET_AUG_* modes of radnet_aug_pointwise_u8


class AdamDesc(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64), ("t", C.c_int32), ("lr", C.c_float)]


SUBSAMPLE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32)
SELECT_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32), C.c_int32)


class HostHooks(C.Structure):
    _fields_ = [("user", C.c_void_p), ("subsample_anchors", SUBSAMPLE_FN), ("select_rois", SELECT_FN)]


class AdamWino(C.Structure):
    """Mirror of `radnet_adam_wino`: a dense [3][3][c][n] kernel inside an optimizer arena and its F(4x4,3x3) filter transform."""
    _fields_ = [("off", C.c_int64), ("c", C.c_int32), ("n", C.c_int32), ("u", C.c_void_p)]


class WgradAdam(C.Structure):
    """Mirror of `radnet_wgrad_adam`: the optimizer block of radnet_conv_wgrad_multi (Adam in the weight gradient's tile epilogue)."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64), ("t", C.c_int32),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("grad_scale", C.c_float)]


class AdamBf16(C.Structure):
    """Mirror of `radnet_adam_bf16`: a conv kernel [k][ldw] inside an optimizer arena and its bf16 image [n][ldk] (bf16-mixed training)."""
    _fields_ = [("off", C.c_int64), ("k", C.c_int32), ("n", C.c_int32), ("ldw", C.c_int32), ("wt", C.c_void_p), ("ldk", C.c_int32)]


class Bf16DgradImage(C.Structure):
    """Mirror of `radnet_bf16_dgrad_image`: a conv kernel [taps*c][ldw] inside an optimizer arena and its dgrad image [c][ldkd] (bf16-train)."""
    _fields_ = [("off", C.c_int64), ("taps", C.c_int32), ("c", C.c_int32), ("n", C.c_int32), ("ldw", C.c_int32), ("wd", C.c_void_p), ("ldkd", C.c_int32)]


class TrainDesc(C.Structure):
    """Mirror of `radnet_train_desc` (field order is the header's)."""
    _d, _i, _vp = C.c_double, C.c_int32, C.c_void_p
    _fields_ = [("img_u8", _vp), ("h", _i), ("w", _i), ("x", _vp),
                ("gt", _vp), ("gt_is_bg", _vp), ("gt_cls", _vp), ("g", _i), ("width", _i), ("height", _i),
                ("anchor_sizes_host", C.POINTER(_d)), ("ns", _i), ("anchor_ratios_host", C.POINTER(_d)), ("nr", _i),
                ("rpn_stride", _d), ("rpn_max_overlap", _d), ("std_scaling", _d),
                ("valid", _vp), ("overlap", _vp), ("regr", _vp), ("best_anchor", _vp), ("n_for_gt", _vp), ("at_scratch", _vp),
                ("h_valid", _vp), ("h_overlap", _vp), ("y_cls", _vp), ("y_regr", _vp),
                ("base_ops", C.POINTER(Op)), ("n_base", _i),
                ("rpn_fwd_ops", C.POINTER(Op)), ("n_rpn_fwd", _i),
                ("rpn_bwd_ops", C.POINTER(Op)), ("n_rpn_bwd", _i),
                ("rpn_refwd_ops", C.POINTER(Op)), ("n_rpn_refwd", _i),
                ("pred", _vp), ("dz", _vp), ("ld_pred", _i), ("fh", _i), ("fw", _i), ("a", _i), ("bce_mode", _i), ("loss_scratch8", _vp), ("rpn_losses", _vp),
                ("rpn_opt", AdamDesc), ("head_opt", AdamDesc), ("world", _i),
                ("wino_w", _vp), ("wino_c", _i), ("wino_n", _i), ("wino_ldw", _i), ("wino_form", _i), ("wino_u", _vp),
                ("anchor_wh_host", C.POINTER(_d)), ("overlap_thresh", _d), ("max_boxes", _i),
                ("R", _vp), ("Rp", _vp), ("Rn", _vp), ("prop_ws", _vp),
                ("rw", _i), ("rh", _i), ("min_overlap", _d), ("max_overlap", _d), ("regr_std_host4", C.POINTER(_d)), ("bg_class", _i),
                ("keep", _vp), ("roi_cls", _vp), ("roi_box", _vp), ("roi_t", _vp), ("roi_iou", _vp),
                ("h_roi_cls", _vp), ("h_n", _vp), ("sel", _vp), ("h_sel", _vp),
                ("head", C.POINTER(HeadDesc)), ("y1", _vp), ("y2", _vp),
                ("head_dz", _vp), ("det_losses", _vp), ("dense_dw", _vp), ("dense_db", _vp), ("dfeat", _vp), ("g_last", _vp),
                ("head_bwd_ops", C.POINTER(Op)), ("n_head_bwd", _i),
                ("head_shift", _vp), ("head_scale", _vp), ("head_bias", _vp), ("head_t0", _vp), ("head_bias_len", C.c_int64),
                ("tail_scratch", _vp), ("head_wino", _vp), ("n_head_wino", C.c_int32)]


def declared_symbols():
    """Names of every function the public header declares."""
    with open(HEADER_PATH) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(radnet_[a-z0-9_]+)\s*\(", text)))


def header_constant(name):
    """Integer value of `#define name <integer>` in the public header (constants a kernel and its tests share)."""
    with open(HEADER_PATH) as f:
        m = re.search(r"^#define\s+%s\s+(-?\d+)\s*$" % re.escape(name), f.read(), flags=re.M)
    if m is None:
        raise RadnetError("include/radnet_hip.h does not define %s" % name)
    return int(m.group(1))


# int32 words in front of / per record of radnet_detect_tail's output
DETECT_HEADER, DETECT_RECORD = header_constant("RADNET_DETECT_HEADER_WORDS"), header_constant("RADNET_DETECT_RECORD_WORDS")


def load_library():
    """dlopen the in-tree library; raises RadnetError (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64; import it first so this library binds to the SAME HIP runtime as the
    # tensors whose pointers it receives (two runtimes in one process do not share devices or allocations)
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RadnetError("libradnet_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(or `make -C rock-art-radnet_amd/csrc`). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    i32, i64, u64, f32, f64, vp = C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double, C.c_void_p
    sig = {
        "radnet_create": (C.c_int, [C.c_int, vp, C.POINTER(vp)]),
        "radnet_destroy": (None, [vp]),
        "radnet_last_error": (C.c_char_p, [vp]),
        "radnet_sync": (C.c_int, [vp]),
        "radnet_set_stream": (C.c_int, [vp, vp]),
        "radnet_version": (C.c_int, []),
        "radnet_set_workspace": (C.c_int, [vp, vp, u64]),
        "radnet_set_autotune": (C.c_int, [vp, C.c_int]),
        "radnet_tuned_shapes": (C.c_int, [vp]),
        "radnet_tune_save": (C.c_int, [vp, C.c_char_p]),
        "radnet_share_tuning": (C.c_int, [vp, vp]),
        "radnet_tune_load": (C.c_int, [vp, C.c_char_p]),
        "radnet_force_config": (C.c_int, [vp, C.c_int, C.c_int, C.c_int]),
        "radnet_force_waves": (C.c_int, [vp, C.c_int]),
        "radnet_set_deterministic": (C.c_int, [vp, C.c_int]),
        "radnet_get_deterministic": (C.c_int, [vp]),
        "radnet_timing_enable": (C.c_int, [vp, C.c_int]),
        "radnet_timing_read": (C.c_int, [vp, C.c_int, C.POINTER(f64), C.POINTER(i64), C.POINTER(f64)]),
        "radnet_timing_reset": (C.c_int, [vp]),
        "radnet_conv_fwd": (C.c_int, [vp, C.POINTER(ConvDesc)]),
        "radnet_conv_fwd_bf16": (C.c_int, [vp, C.POINTER(ConvDesc), vp, i32]),
        "radnet_conv_fwd_bf16_split": (C.c_int, [vp, C.POINTER(ConvDesc), vp, i32, i32]),
        "radnet_conv_bf16_pick_split": (i32, [C.c_int64, i32, i32]),
        "radnet_conv_bf16_tile_shape": (i64, [i64, i32, C.POINTER(i32), C.POINTER(i32)]),
        "radnet_weights_to_bf16": (C.c_int, [vp, vp, i32, i32, i32, vp, i32]),
        "radnet_weights_to_bf16_dgrad": (C.c_int, [vp, vp, i32, i32, i32, i32, vp, i32]),
        "radnet_weights_to_bf16_dgrad_arena": (C.c_int, [vp, vp, i64, C.POINTER(Bf16DgradImage), i32]),
        "radnet_conv_dgrad_bf16": (C.c_int, [vp, C.POINTER(ConvDesc), vp, i32]),
        "radnet_conv_dgrad_bf16_split": (C.c_int, [vp, C.POINTER(ConvDesc), vp, i32, i32]),
        "radnet_conv_wgrad_bf16": (C.c_int, [vp, C.POINTER(ConvDesc), i32]),
        "radnet_dgrad_bf16_pick_split": (i32, [C.c_int64, i32, i32]),
        "radnet_wgrad_bf16_pick_split": (i32, [C.c_int64, i32, i32]),
        "radnet_conv_dgrad": (C.c_int, [vp, C.POINTER(ConvDesc)]),
        "radnet_gemm_batched": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32]),
        "radnet_winograd_filter": (C.c_int, [vp, vp, i32, i32, i32, vp]),
        "radnet_winograd_input": (C.c_int, [vp, vp, i32, i32, i32, i32, vp]),
        "radnet_winograd_output": (C.c_int, [vp, vp, i32, i32, i32, i32, vp, vp, i32, vp, i32]),
        "radnet_winograd_dy": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, vp, vp]),
        "radnet_wgrad_batched": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32]),
        "radnet_winograd_filter_grad": (C.c_int, [vp, vp, i32, i32, i32, vp, i32]),
        "radnet_winograd4_filter": (C.c_int, [vp, vp, i32, i32, i32, vp]),
        "radnet_winograd4_input": (C.c_int, [vp, vp, i32, i32, i32, i32, vp]),
        "radnet_winograd4_output": (C.c_int, [vp, vp, i32, i32, i32, i32, vp, vp, i32, vp, i32]),
        "radnet_winograd4_dy": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, vp, vp]),
        "radnet_winograd4_filter_grad": (C.c_int, [vp, vp, i32, i32, i32, vp, i32]),
        "radnet_adam_step_fused": (C.c_int, [vp, vp, vp, vp, vp, C.c_int64, i32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, i32,
                                            C.c_int64, C.c_int64, vp, vp, vp, C.POINTER(AdamWino), i32]),
        "radnet_adam_step_tail": (C.c_int, [vp, vp, vp, vp, vp, C.c_int64, i32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, i32,
                                           C.c_int64, C.c_int64, vp, vp, vp, C.POINTER(AdamWino), i32, C.c_int64]),
        "radnet_adam_step_bf16": (C.c_int, [vp, vp, vp, vp, vp, C.c_int64, i32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, i32,
                                           C.c_int64, C.c_int64, vp, vp, vp, C.POINTER(AdamBf16), i32]),
        "radnet_conv_wgrad": (C.c_int, [vp, C.POINTER(ConvDesc)]),
        "radnet_conv_bwd": (C.c_int, [vp, C.POINTER(ConvDesc)]),
        "radnet_conv_wgrad_multi": (C.c_int, [vp, C.POINTER(ConvDesc), i32, C.POINTER(WgradAdam)]),
        "radnet_conv_fwd_pair": (C.c_int, [vp, C.POINTER(ConvDesc), C.POINTER(ConvDesc)]),
        "radnet_conv_bottleneck": (C.c_int, [vp, C.POINTER(ConvDesc), C.POINTER(ConvDesc), C.POINTER(ConvDesc)]),
        "radnet_colsum": (C.c_int, [vp, vp, i32, i32, i32, vp, vp, i32]),
        "radnet_maxpool_fwd": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, i32]),
        "radnet_roi_resize_fwd": (C.c_int, [vp, vp, i32, i32, i32, vp, i32, i32, vp]),
        "radnet_roi_resize_bwd": (C.c_int, [vp, vp, i32, i32, i32, vp, i32, i32, vp]),
        "radnet_avgpool_fwd": (C.c_int, [vp, vp, i32, i32, i32, vp]),
        "radnet_avgpool_bwd_relu": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
        "radnet_dense_heads_fwd": (C.c_int, [vp, vp, i32, i32, vp, i32, vp, i32, i32, vp, vp]),
        "radnet_dense_heads_bwd": (C.c_int, [vp, vp, vp, i32, i32, vp, i32, i32, vp, vp, vp, i32]),
        "radnet_head_tail_scratch_bytes": (u64, [i32]),
        "radnet_head_tail_fwd": (C.c_int, [vp, vp, i32, i32, i32, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]),
        "radnet_rpn_loss": (C.c_int, [vp, vp, i32, vp, vp, i32, i32, i32, vp, i32, vp, vp]),
        "radnet_det_loss": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp]),
        "radnet_adam_step": (C.c_int, [vp, vp, vp, vp, vp, i64, i32, f32, f32, f32, f32, f32, i32]),
        "radnet_adam_step_affine": (C.c_int, [vp, vp, vp, vp, vp, i64, i32, f32, f32, f32, f32, f32, i32, i64, i64, vp, vp, vp]),
        "radnet_affine_vec": (C.c_int, [vp, vp, vp, vp, vp, i64]),
        "radnet_relu_mask": (C.c_int, [vp, vp, vp, i64]),
        "radnet_scatter_strided": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp]),
        "radnet_proposals_ws_bytes": (u64, [i64]),
        "radnet_rpn_to_roi": (C.c_int, [vp, vp, i32, i32, i32, i32, C.POINTER(f64), f64, i32, f64, i32, vp, vp, vp, vp]),
        "radnet_nms": (C.c_int, [vp, vp, vp, i32, f64, i32, vp, vp, vp]),
        "radnet_anchor_targets": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, C.POINTER(f64), i32, C.POINTER(f64), i32,
                                            f64, f64, vp, vp, vp, vp, vp, vp]),
        "radnet_anchor_targets_pack": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, f64, vp, vp]),
        "radnet_roi_targets": (C.c_int, [vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, f64, f64, f64, C.POINTER(f64), i32,
                                         vp, vp, vp, vp, vp, vp]),
        "radnet_roi_batch_pack": (C.c_int, [vp, vp, i32, vp, vp, vp, i32, i32, vp, vp, vp]),
        "radnet_host_choice_round": (i64, [vp, vp, vp, vp, i64, vp, i64, vp, vp]),
        "radnet_preprocess_bgr": (C.c_int, [vp, vp, i32, i32, i32, vp]),
        "radnet_resize_bicubic_u8": (C.c_int, [vp, vp, i32, i32, vp, i32, i32, i32]),
        "radnet_resize_bicubic_window_u8": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, i32, vp, i32, i32, i32]),
        "radnet_warp_affine_u8": (C.c_int, [vp, vp, i32, i32, i32, vp, i32, i32, vp, vp]),
        "radnet_aug_gather_u8": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
        "radnet_aug_extent_u8": (C.c_int, [vp, vp, i32, i32, vp]),
        "radnet_aug_histogram_u8": (C.c_int, [vp, vp, i32, i32, i32, vp]),
        "radnet_aug_pointwise_u8": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, f64, f64, u64, C.c_uint32]),
        "radnet_png_unfilter_u8": (C.c_int, [vp, vp, i32, i32, i32]),
        "radnet_png_plan_segments": (C.c_int, [vp, i64, i32, i32, i32, vp, i32]),
        "radnet_png_unfilter_segments_u8": (C.c_int, [vp, vp, i64, vp, vp, i32, i32]),
        "radnet_png_expand_bgr_u8": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, i32, i32]),
        "radnet_png_filter_rows_u8": (C.c_int, [vp, vp, i32, i32, i32, i64, i32, vp]),
        "radnet_deflate_rle_scan_u8": (C.c_int, [vp, vp, i64, vp, vp]),
        "radnet_deflate_rle_emit_u8": (C.c_int, [vp, vp, i64, vp, vp, i32, i32, vp, i64, vp]),
        "radnet_deflate_piece_cap": (i64, [vp, i32, i32]),
        "radnet_deflate_pack": (C.c_int, [vp, vp, i64, vp, i32, vp, i64, vp]),
        "radnet_deflate_build_code": (C.c_int, [vp, vp, vp, i32, C.POINTER(i32)]),
        "radnet_deflate_lz_scan_u8": (C.c_int, [vp, vp, i64, i32, vp, vp, vp, vp]),
        "radnet_deflate_lz_emit_u8": (C.c_int, [vp, vp, i64, vp, vp, vp, vp, i32, vp, i64, vp]),
        "radnet_deflate_build_codes_lz": (C.c_int, [vp, vp, vp, vp, vp, i32, C.POINTER(i32)]),
        "radnet_deflate_lz_piece_cap": (i64, [vp, vp, i32]),
        "radnet_deflate_stream_bits": (i64, [vp, vp, vp, vp, i32, i32, i64]),
        "radnet_png_check_crcs": (C.c_int, [vp, i64, vp, vp, i32, i32]),
        "radnet_inflate_find_blocks": (C.c_int, [vp, vp, i64, i64, vp, i32, vp]),
        "radnet_inflate_rle_measure": (C.c_int, [vp, vp, i64, vp, i32]),
        "radnet_inflate_chain": (C.c_int, [vp, i32, i64, i64, i64, vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "radnet_inflate_rle_emit": (C.c_int, [vp, vp, i64, vp, i32, vp, i64]),
        "radnet_inflate_lz_measure": (C.c_int, [vp, vp, i64, vp, i32]),
        "radnet_inflate_lz_chain": (C.c_int, [vp, i32, i64, i64, i64, vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "radnet_inflate_lz_emit": (C.c_int, [vp, vp, i64, vp, i32, vp, vp, i64]),
        "radnet_inflate_lz_resolve": (C.c_int, [vp, vp, i64, i32, vp]),
        "radnet_inflate_lz_gather": (C.c_int, [vp, vp, vp, i64]),
        "radnet_inflate_streams_check": (C.c_int, [vp, i32, i64, i64, C.POINTER(i32), C.c_char_p, i32]),
        "radnet_inflate_find_blocks_many": (C.c_int, [vp, vp, i64, vp, vp, i32, vp, i32, vp]),
        "radnet_inflate_rle_measure_many": (C.c_int, [vp, vp, i64, vp, vp, i32, vp, i32]),
        "radnet_inflate_lz_measure_many": (C.c_int, [vp, vp, i64, vp, vp, i32, vp, i32]),
        "radnet_inflate_rle_emit_many": (C.c_int, [vp, vp, i64, vp, vp, i32, vp, i32, vp, i64]),
        "radnet_inflate_lz_emit_many": (C.c_int, [vp, vp, i64, vp, vp, i32, vp, i32, vp, vp, i64]),
        "radnet_png_gather_column_u8": (C.c_int, [vp, vp, i64, vp, vp, vp, i32, vp]),
        "radnet_png_plan_segments_column": (C.c_int, [vp, i64, i32, i32, i32, vp, i32]),
        "radnet_png_plan_tiles": (C.c_int, [i32, i32, i32, vp]),
        "radnet_png_tiles_on_sweep": (C.c_int, [i32, i32, i32, i32, vp, i32]),
        "radnet_png_unfilter_tiles_u8": (C.c_int, [vp, vp, i64, vp, vp, i32, i32]),
        "radnet_png_unfilter_tiles_width_u8": (C.c_int, [vp, vp, i64, vp, vp, i32, i32, i32]),
        "radnet_crc32_shift": (C.c_uint32, [i64]),
        "radnet_crc32_combine": (C.c_uint32, [C.c_uint32, C.c_uint32, i64]),
        "radnet_crc32_plan_segments": (C.c_int, [vp, i32, i64, i32, vp, C.POINTER(i32), C.c_char_p, i32]),
        "radnet_crc32_segments": (C.c_int, [vp, vp, i64, vp, vp, i32, vp, vp]),
        "radnet_png_plan_join": (C.c_int, [vp, i32, i64, i64, i32, vp, C.POINTER(i32), C.c_char_p, i32]),
        "radnet_png_join_u8": (C.c_int, [vp, vp, i64, vp, vp, i32, vp, i64]),
        "radnet_draw_rects_u8": (C.c_int, [vp, vp, i32, i32, i64, vp, vp, i32]),
        "radnet_draw_list_u8": (C.c_int, [vp, vp, i32, i32, i64, vp, vp, i32, vp, vp, i32]),
        "radnet_draw_glyph_rows": (C.c_int, [i32, vp]),
        "radnet_draw_scene_u8": (C.c_int, [vp, vp, i32, i32, i64, vp, vp, i32, vp, vp, i32]),
        "radnet_draw_scene_check": (C.c_int, [vp, i32, vp, i32, C.POINTER(i32), C.c_char_p, i32]),
        "radnet_grey3_u8": (C.c_int, [vp, vp, vp, i32, i32, i64, i64]),
        "radnet_score_levels_u8": (C.c_int, [vp, vp, i32, i32, i32, i32, vp]),
        "radnet_heat_paint_u8": (C.c_int, [vp, vp, i32, i32, i64, vp, i64, vp, vp, i32, vp, i32, i32]),
        "radnet_heat_check": (C.c_int, [vp, i32, i64, i32, i32, C.POINTER(i32), C.c_char_p, i32]),
        "radnet_fill_zero": (C.c_int, [vp, vp, u64]),
        "radnet_copy_bytes": (C.c_int, [vp, vp, vp, C.c_uint64]),
        "radnet_program_run": (C.c_int, [vp, C.POINTER(Op), i32]),
        "radnet_rpn_forward": (C.c_int, [vp, C.POINTER(Op), i32, C.POINTER(Op), i32]),
        "radnet_predict_tile": (C.c_int, [vp, C.POINTER(TileDesc)]),
        "radnet_detect_tail_out_bytes": (u64, [i32]),
        "radnet_detect_tail": (C.c_int, [vp, C.POINTER(DetectTailDesc)]),
        "radnet_rois_from_proposals": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
        "radnet_predict_tile_detect": (C.c_int, [vp, C.POINTER(TileDesc), C.POINTER(DetectTailDesc)]),
        "radnet_final_nms_ws_bytes": (u64, [i32, i32]),
        "radnet_final_nms": (C.c_int, [vp, C.POINTER(FinalNmsDesc)]),
        "radnet_scan_merge_out_bytes": (u64, [i32, i32]),
        "radnet_scan_merge_ws_bytes": (u64, [i32, i32, i32, i32, i32]),
        "radnet_scan_merge": (C.c_int, [vp, C.POINTER(ScanMergeDesc)]),
        "radnet_scan_merge_check": (C.c_int, [vp, i32, i64, i32, C.POINTER(i32), C.POINTER(i32), C.c_char_p, i32]),
        "radnet_train_step": (C.c_int, [vp, C.POINTER(TrainDesc), C.POINTER(HostHooks), C.POINTER(C.c_float), C.POINTER(i32)]),
        "radnet_comm_unique_id": (C.c_int, [C.c_char_p]),
        "radnet_comm_init": (C.c_int, [vp, i32, i32, C.c_char_p]),
        "radnet_comm_destroy": (C.c_int, [vp]),
        "radnet_allreduce_grads": (C.c_int, [vp, vp, i64]),
        "radnet_comm_stats": (C.c_int, [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "radnet_chain_build": (C.c_int, [vp, vp, i32, i32, C.POINTER(vp)]),
        "radnet_chain_run": (C.c_int, [vp, vp]),
        "radnet_chain_error": (C.c_uint32, [vp]),
        "radnet_chain_status": (C.c_int, [vp, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(f64), C.POINTER(f64)]),
        "radnet_chain_destroy": (None, [vp]),
        "radnet_chain_peek": (C.c_int, [vp, i32, C.POINTER(C.c_uint32), i32]),
        "radnet_chain_check": (C.c_int, [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.c_char_p, i32]),
        "radnet_scale": (C.c_int, [vp, vp, i64, f32]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)          # AttributeError here = header/binding drift: fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def glyph_rows(code):
    """The 8 row bytes of the draw list's glyph of `code` (radnet_draw_glyph_rows: host only, no context, no device), top row
    first; the dot of column c is (row >> (4 - c)) & 1.  The table stands in csrc/draw_font.h and nowhere else."""
    rows = (C.c_uint8 * 8)()
    rc = load_library().radnet_draw_glyph_rows(int(code), rows)
    if rc != 0:
        raise RadnetError("radnet_draw_glyph_rows: no glyph for the code 0x%02X (the font has 0x20..0x7E)" % int(code))
    return bytes(rows)


def draw_scene_check(table, chars=b"", count=None, n_chars=None):
    """radnet_draw_scene_check (host only, no context, no device) on a table of radnet_prim rows -- a NumPy array of 8 int32 per
    entry, or None for a null table -- and a character pool (bytes, or None for a null pool): (rc, index of the bad entry or -1,
    the message).  count and n_chars default to the sizes of what is passed."""
    import numpy as np
    rows = np.zeros((0, 8), np.int32) if table is None else np.ascontiguousarray(table).view(np.int32).reshape(-1, 8)
    pool = np.frombuffer(bytes(chars or b""), np.uint8)
    bad, msg = C.c_int32(-2), C.create_string_buffer(256)
    rc = load_library().radnet_draw_scene_check(rows.ctypes.data if len(rows) else None, len(rows) if count is None else int(count),
                                                pool.ctypes.data if len(pool) else None, len(pool) if n_chars is None else int(n_chars),
                                                C.byref(bad), msg, len(msg))
    return rc, bad.value, msg.value.decode()


def heat_check(table, pool_len, h, w, count=None):
    """radnet_heat_check (host only, no context, no device) on a table of radnet_heat_place rows -- a NumPy array of 32 bytes per
    entry, or None for a null table -- for an image of h x w pixels and a pool of pool_len bytes: (rc, index of the bad entry or
    -1, the message).  count defaults to the table's length."""
    import numpy as np
    rows = np.zeros((0, 32), np.uint8) if table is None else np.ascontiguousarray(table).view(np.uint8).reshape(-1, 32)
    bad, msg = C.c_int32(-2), C.create_string_buffer(256)
    rc = load_library().radnet_heat_check(rows.ctypes.data if len(rows) else None, len(rows) if count is None else int(count), int(pool_len), int(h),
                                          int(w), C.byref(bad), msg, len(msg))
    return rc, bad.value, msg.value.decode()


def crc32_shift(length):
    """radnet_crc32_shift (host only): x^(8 * length) mod the CRC-32 polynomial, as a reflected register."""
    return int(load_library().radnet_crc32_shift(int(length)))


def crc32_combine(crc1, crc2, len2):
    """radnet_crc32_combine (host only): zlib's crc32_combine."""
    return int(load_library().radnet_crc32_combine(int(crc1) & 0xffffffff, int(crc2) & 0xffffffff, int(len2)))


def crc32_plan_segments(table, n, misalign=0, count=None):
    """radnet_crc32_plan_segments (host only, no context, no device) on a table of radnet_crc32_segment rows -- a NumPy array of 24
    bytes per entry, or None for a null table -- for a buffer of n bytes that stands `misalign` bytes behind a 16-byte boundary:
    (rc, spans, ws_bytes, index of the bad entry or -1, the message).  count defaults to the table's length."""
    import numpy as np
    rows = np.zeros((0, 24), np.uint8) if table is None else np.ascontiguousarray(table).view(np.uint8).reshape(-1, 24)
    plan, bad, msg = (C.c_int64 * 2)(-1, -1), C.c_int32(-2), C.create_string_buffer(256)
    rc = load_library().radnet_crc32_plan_segments(rows.ctypes.data if len(rows) else None, len(rows) if count is None else int(count), int(n),
                                                   int(misalign), C.cast(plan, C.c_void_p), C.byref(bad), msg, len(msg))
    return rc, plan[0], plan[1], bad.value, msg.value.decode()


def png_plan_join(table, file_len, n, misalign=0, count=None):
    """radnet_png_plan_join (host only, no context, no device) on a table of radnet_png_piece rows -- a NumPy array of 24 bytes per
    entry, or None for a null table -- of a file of file_len bytes, for an output of n bytes that stands `misalign` bytes behind a
    16-byte boundary: (rc, grains, spans, index of the bad entry or -1, the message).  count defaults to the table's length."""
    import numpy as np
    rows = np.zeros((0, 24), np.uint8) if table is None else np.ascontiguousarray(table).view(np.uint8).reshape(-1, 24)
    plan, bad, msg = (C.c_int64 * 2)(-1, -1), C.c_int32(-2), C.create_string_buffer(256)
    rc = load_library().radnet_png_plan_join(rows.ctypes.data if len(rows) else None, len(rows) if count is None else int(count), int(file_len), int(n),
                                             int(misalign), C.cast(plan, C.c_void_p), C.byref(bad), msg, len(msg))
    return rc, plan[0], plan[1], bad.value, msg.value.decode()


def inflate_streams_check(table, z_len, out_len, count=None):
    """radnet_inflate_streams_check (host only, no context, no device) on a table of radnet_inflate_stream rows -- a NumPy array of
    32 bytes per entry, or None for a null table -- for z_len compressed and out_len inflated bytes: (rc, index of the bad stream
    or -1, the message).  count defaults to the table's length."""
    import numpy as np
    rows = np.zeros((0, 32), np.uint8) if table is None else np.ascontiguousarray(table).view(np.uint8).reshape(-1, 32)
    bad, msg = C.c_int32(-2), C.create_string_buffer(256)
    rc = load_library().radnet_inflate_streams_check(rows.ctypes.data if len(rows) else None, len(rows) if count is None else int(count), int(z_len),
                                                     int(out_len), C.byref(bad), msg, len(msg))
    return rc, bad.value, msg.value.decode()


def scan_merge_check(table, pool_words, slot_rows, count=None):
    """radnet_scan_merge_check (host only, no context, no device) on a table of radnet_scan_tile rows -- a NumPy array of 16 bytes
    per entry, or None for a null table -- for a pool of pool_words int32 words whose slots hold slot_rows rows:
    (rc, number of images, index of the bad entry or -1, the message).  count defaults to the table's length."""
    import numpy as np
    rows = np.zeros((0, 16), np.uint8) if table is None else np.ascontiguousarray(table).view(np.uint8).reshape(-1, 16)
    n_images, bad, msg = C.c_int32(-2), C.c_int32(-2), C.create_string_buffer(256)
    rc = load_library().radnet_scan_merge_check(rows.ctypes.data if len(rows) else None, len(rows) if count is None else int(count), int(pool_words),
                                                int(slot_rows), C.byref(n_images), C.byref(bad), msg, len(msg))
    return rc, n_images.value, bad.value, msg.value.decode()


def _ptr(t):
    """Device pointer of a torch tensor (or None / int passthrough)."""
    if t is None:
        return None
    if isinstance(t, int):
        return t
    return t.data_ptr()


class Context:
    """One `radnet_ctx` bound to a device and a HIP stream (default: torch's current stream)."""

    def __init__(self, device_index=0, stream_handle=None):
        import torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise RadnetError("no MI355X visible: the RADNet HIP path has no CPU fallback")
        if stream_handle is None:
            with torch.cuda.device(device_index):
                stream_handle = torch.cuda.current_stream().cuda_stream
        h = C.c_void_p()
        rc = self.lib.radnet_create(int(device_index), C.c_void_p(stream_handle), C.byref(h))
        if rc != 0:
            raise RadnetError("radnet_create failed with code %d (needs a gfx950 device)" % rc)
        self.h = h
        self.device_index = device_index
        self.stream_handle = stream_handle
        self.timing_on = False

    def close(self):
        if getattr(self, "h", None):
            self.lib.radnet_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc, what=""):
        if rc != 0:
            msg = self.lib.radnet_last_error(self.h)
            raise RadnetError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))

    def call(self, name, *args):
        fn = getattr(self.lib, name)
        self.check(fn(self.h, *[_ptr(a) if hasattr(a, "data_ptr") else a for a in args]), name)

    def sync(self):
        self.check(self.lib.radnet_sync(self.h), "radnet_sync")

    def set_stream(self, stream_handle):
        self.check(self.lib.radnet_set_stream(self.h, C.c_void_p(stream_handle)), "radnet_set_stream")
        self.stream_handle = stream_handle

    # timing of the GEMM-class launches (HIP events on the ctx stream)
    def timing(self, enable):
        self.check(self.lib.radnet_timing_enable(self.h, 1 if enable else 0), "timing_enable")
        self.timing_on = bool(enable)

    def timing_reset(self):
        self.check(self.lib.radnet_timing_reset(self.h), "timing_reset")

    def timing_read(self, cls):
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        self.check(self.lib.radnet_timing_read(self.h, cls, C.byref(ms), C.byref(n), C.byref(fl)), "timing_read")
        return ms.value, n.value, fl.value
