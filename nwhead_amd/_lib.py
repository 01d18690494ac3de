"""ctypes binding of libnwhead_hip.so (the C ABI in include/nwhead_hip.h).

There is NO fallback: if the shared library is missing, or a tensor is not on a HIP device, the
ops raise.  Build with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C nwhead_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# NW_HIP_LIB: another build of the same library (A/B timing of kernel variants on one device)
LIB_PATH = os.environ.get("NW_HIP_LIB") or os.path.join(_HERE, "csrc", "libnwhead_hip.so")

SCORE_KINDS = {"euclidean": 0, "hypersphere_euclidean": 1, "cosine": 2, "dotproduct": 3, "clip": 4}

_p = C.c_void_p
_i64 = C.c_int64
_int = C.c_int
_sz = C.c_size_t

# name -> (restype, argtypes); mirrors include/nwhead_hip.h one to one
SIGNATURES = {
    "nw_abi_version": (_int, []),
    "nw_status_string": (C.c_char_p, [_int]),
    "nw_device_check": (_int, []),
    "nw_scores_f32": (_int, [_p, _p, _p, _i64, _i64, _i64, _int, _p, _int, _p]),
    "nw_fwd_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "nw_row_norm2_f32": (_int, [_p, _p, _i64, _i64, _p]),
    "nw_split_rows_f16x2": (_int, [_p, _p, _p, _p, _i64, _i64, _p]),
    "nw_pack_rows_f16": (_int, [_p, _p, _p, _p, _i64, _i64, _p]),
    "nw_bank_update_rows_f32": (_int, [_p, _p, _i64, _i64, C.c_float, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _p]),
    "nw_fwd_f32": (_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _i64, _i64, _i64, _i64, _int, _p, _int, _int, _p, _p]),
    "nw_fwd_partial_f32": (_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _i64, _i64, _i64, _i64, _int, _p, _p, _p]),
    "nw_merge_finalize_f32": (_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _p, _i64, _p]),
    "nw_bank_tables_bytes": (_sz, [_i64]),
    "nw_bank_tables_build": (_int, [_p, _i64, _i64, _p, _sz, _p]),
    "nw_bwd_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _int, _int]),
    "nw_bwd_f32": (_int, [_p] * 10 + [_p, _sz, _i64, _i64, _i64, _i64, _int, _p, _int, _int, _p]),
    "nw_bwd_uses_split": (_int, [_i64, _i64, _i64, _i64, _int]),
    "nw_bwd_bank_f32": (_int, [_p] * 13 + [_p, _sz, _i64, _i64, _i64, _i64, _int, _p, _int, _int, _p]),
    "nw_support_influence_f32": (_int, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _p]),
    "nw_aggregate_f32": (_int, [_p] * 5 + [_i64, _i64, _i64, _int, _p]),
    "nw_aggregate_bwd_f32": (_int, [_p] * 6 + [_i64, _i64, _i64, _int, _p]),
    "nw_fwd_influence_f32": (_int, [_p] * 11 + [_sz, _i64, _i64, _i64, _i64, _int, _p, _p, _p]),
    "nw_topk_f32": (_int, [_p, _p, _p, _i64, _i64, _i64, _p]),
    "nw_knn_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "nw_scores_use_split": (_int, [_i64, _i64, _i64]),
    "nw_knn_f32": (_int, [_p, _p, _p, _p, _p, _p, _p, _sz, _i64, _i64, _i64, _i64, _int, _p, _p]),
    "nw_knn_window_f32": (_int, [_p, _p, _p, _p, _p, _p, _int, _p, _p, _p, _sz, _i64, _i64, _i64, _i64, _int, _p, _p]),
    "nw_fwd_window_f32": (_int, [_p, _p, _p, _p, _p, _p, _p, _int, _p, _p, _p, _sz, _i64, _i64, _i64, _i64, _int, _p, _p]),
    "nw_fwd_weighted_f32": (_int, [_p, _p, _p, _p, _p, _p, _p, _p, _int, _p, _p, _p, _sz, _i64, _i64, _i64, _i64, _int, _p, _p]),
    "nw_bwd_query_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _int]),
    "nw_bwd_query_f32": (_int, [_p, _p, _p, _p, _p, _p, _p, _int, _p, _p, _p, _p, _p, _p, _sz, _i64, _i64, _i64, _i64, _int, _p, _int, _p]),
    "nw_bwd_query_weighted_f32": (_int, [_p, _p, _p, _p, _p, _p, _p, _p, _int, _p, _p, _p, _p, _p, _p, _sz, _i64, _i64, _i64, _i64, _int, _p,
                                         _int, _p]),
    "nw_bwd_logw_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _int, _int]),
    "nw_bwd_query_logw_f32": (_int, [_p, _p, _p, _p, _p, _p, _p, _p, _int, _p, _p, _p, _p, _p, _p, _p, _sz, _i64, _i64, _i64, _i64, _int,
                                     _p, _int, _p]),
    "nw_fwd_values_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _int]),
    "nw_fwd_values_f32": (_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _int, _p, _p, _p, _sz, _i64, _i64, _i64, _i64, _int, _p, _int, _p]),
    "nw_bwd_values_query_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _int]),
    "nw_bwd_values_query_f32": (_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _int, _p, _p, _p, _p, _p, _p, _sz, _i64, _i64, _i64, _i64,
                                       _int, _p, _int, _p]),
    "nw_bwd_values_support_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _int, _int]),
    "nw_bwd_values_support_f32": (_int, [_p, _p, _p, _p, _p, _p, _p, _p, _int, _p, _p, _p, _p, _p, _p, _sz, _i64, _i64, _i64, _i64,
                                         _int, _p, _int, _p]),
    "nw_bwd_bank_support_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _int]),
    "nw_bwd_bank_support_f32": (_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _int, _p, _p, _p, _p, _p, _sz, _i64, _i64, _i64, _i64,
                                       _int, _p, _int, _p]),
    "nw_bwd_values_bank_support_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _int]),
    "nw_bwd_values_bank_support_f32": (_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _int, _p, _p, _p, _p, _p, _sz, _i64, _i64, _i64,
                                              _i64, _int, _p, _int, _p]),
    "nw_influence_select_f32":(_int, [_p] * 8 + [_i64, _i64, _i64, _i64, _p]),
    "nw_knn_f16_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "nw_knn_f16": (_int, [_p, _p, _p, _p, _p, _p, _p, _sz, _i64, _i64, _i64, _i64, _int, _p, _p, _p]),
    "nw_knn_merge_f32": (_int, [_p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _p, _p, _p, _p, _p]),
    "nw_scale_shift_relu_f32": (_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _int, _p]),
    "nw_bias_act_nhwc_f32": (_int, [_p, _p, _p, _int, _p, _i64, _i64, _p]),
    "nw_scale_shift_relu_avgpool2_f32": (_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _int, _p]),
    "nw_conv3x3_workgroups": (_i64, [_i64, _i64, _i64, _i64, _i64]),
    "nw_conv3x3_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _i64]),
    "nw_conv3x3_f32": (_int, [_p, _i64, _p, _p, _p, _i64, _int, _p, _i64, _p, _sz, _i64, _i64, _i64, _i64, _i64, _p]),
    "nw_conv1x1_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "nw_conv1x1_f32": (_int, [_p, _i64, _p, _p, _int, _p, _p, _int, _p, _i64, _p, _sz, _i64, _i64, _i64, _i64, _p]),
    "nw_bn_relu_train_fwd_f32": (_int, [_p] * 10 + [_i64, _i64, _i64, _i64, C.c_float, C.c_float, _int, _p]),
    "nw_bn_relu_train_bwd_f32": (_int, [_p] * 12 + [_i64, _i64, _i64, _i64, _i64, _int, _p]),
    "nw_absmax_f32": (_int, [_p, _i64, _p, _p]),
    "nw_to_nhwc_pad_f32": (_int, [_p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p]),
    "nw_conv2d_nhwc_supported": (_int, [_i64] * 9),
    "nw_conv2d_nhwc_f16x2": (_int, [_p, _p, _p, _p, _p, _p, _int, _p, _p] + [_i64] * 11 + [_p, _p]),
    "nw_conv2d_nhwc_moments_groups": (_i64, [_i64] * 9),
    "nw_stem7x7s2_relu_maxpool_supported": (_int, [_i64] * 4),
    "nw_stem7x7s2_relu_maxpool_f16x2": (_int, [_p] * 7 + [_i64] * 4 + [_p]),
    "nw_bn_relu_avgpool2x2_nhwc_f32": (_int, [_p, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _p]),
    "nw_add_relu_f32": (_int, [_p, _p, _p, _p, _i64, _p]),
    "nw_relu_bwd_f32": (_int, [_p, _p, _p, _p, _i64, _p]),
    "nw_bn_nhwc_moments_f32": (_int, [_p, _i64, _i64, _i64, C.c_float, _p, _p, _p, _p, _sz, _p]),
    "nw_bn_nhwc_moments_from_partials_f32": (_int, [_p, _i64, _i64, C.c_float, _p, _p, _p, _p]),
    "nw_bn_nhwc_moments_minmax_f32": (_int, [_p, _i64, _i64, _i64, C.c_float, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "nw_bn_nhwc_minmax_workspace_bytes": (_sz, [_i64, _i64]),
    "nw_bn_nhwc_prep_from_partials_f32": (_int, [_p, _i64, _i64, C.c_float, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, C.c_float, _int,
                                                 _p, _p, _p]),
    "nw_bn_nhwc_prep_window_from_partials_f32": (_int, [_p, _i64, _i64, _i64, _i64, _i64, C.c_float, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                                        _p, C.c_float, _int, _p, _p, _p]),
    "nw_bn_nhwc_prep_f32": (_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, C.c_float, _int, _i64, _i64, _p, _p, _p]),
    "nw_conv2d_nhwc_bnrelu_f16x2": (_int, [_p] * 3 + [_i64] + [_p] * 3 + [_int, _p, _p] + [_i64] * 11 + [_p, _p]),
    "nw_bn_relu_nhwc_apply_f32": (_int, [_p, _i64] + [_p] * 8 + [C.c_float, _p, _p, _i64, _i64, _int, _p]),
    "nw_split_conv_weights_f16x2": (_int, [_p, _i64, _i64, _p, _p, _p]),
    "nw_conv2d_nhwc_wgrad_supported": (_int, [_i64] * 9),
    "nw_conv2d_nhwc_wgrad_workspace_bytes": (_sz, [_i64] * 9),
    "nw_conv2d_nhwc_wgrad_f16x2": (_int, [_p, _p, _p, _p, _p, _p, _sz] + [_i64] * 11 + [_p]),
    "nw_conv_zero_page": (_p, []),
    "nw_conv2d_nhwc_wgrad_batch_workspace_bytes": (_sz, [_p, _i64]),
    "nw_conv2d_nhwc_wgrad_batch_f16x2": (_int, [_p, _i64, _p, _sz, _p]),
    "nw_bn_nhwc_workspace_bytes": (_sz, [_i64, _i64]),
    "nw_bn_relu_nhwc_train_fwd_f32": (_int, [_p, _i64] + [_p] * 10 + [_sz, _i64, _i64, C.c_float, C.c_float, _int, _p]),
    "nw_bn_relu_nhwc_train_bwd_f32": (_int, [_p, _i64] + [_p] * 9 + [_i64, _i64, _p, _p, _sz, _i64, _i64, _int, _p]),
    "nw_avgpool2x2_nhwc_f32": (_int, [_p, _i64, _p, _i64, _i64, _i64, _i64, _i64, _p]),
    "nw_avgpool2x2_nhwc_bwd_f32": (_int, [_p, _i64, _p, _i64, _i64, _i64, _i64, _i64, _p]),
    "nw_maxpool3x3s2_nhwc_f32": (_int, [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i64, _p]),
    "nw_maxpool3x3s2_nhwc_bwd_f32": (_int, [_p, _i64, _p, _p, _i64, _i64, _i64, _i64, _i64, _p]),
    "nw_sgd_step_f32": (_int, [_p, _i64, C.c_float, C.c_float, C.c_float, _int, _int, _p]),
    "nw_debug_set": (_int, [C.c_char_p, _int]),
    "nw_debug_tile_timing": (_int, [_int]),
    "nw_debug_tile_timing_read": (_int, [C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "nw_debug_fwd_plan": (_int, [_i64, _i64, _i64, _i64, _int, _int, _int, _int, _int, _int, _int, _p]),
    "nw_debug_fwd_layout": (_int, [_i64, _i64, _i64, _i64, _p]),
    "nw_debug_bwd_plan": (_int, [_i64, _i64, _i64, _i64, _int, _p]),
}

_lib = None


class NWHipError(RuntimeError):
    pass


def load():
    """Load the shared library once; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NWHipError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run __graft_entry__.build() "
            "(or `make -C nwhead_amd/csrc`). There is no CPU fallback.")
    # torch ships its own HIP runtime (torch/lib/libamdhip64.so); it must be in the process before this
    # library's NEEDED libamdhip64 is resolved, or the loader pulls /opt/rocm's copy in and the process ends
    # up with two runtimes, the second of which cannot open the device (nw_device_check: no gfx950 device).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.nw_abi_version() != 2:
        raise NWHipError("libnwhead_hip.so ABI version mismatch")
    _lib = lib
    sync_knobs()
    return lib


class WgradJob(C.Structure):
    """nw_wgrad_job (include/nwhead_hip.h)."""
    _fields_ = [("x", C.c_void_p), ("amax_x", C.c_void_p), ("gy", C.c_void_p), ("amax_g", C.c_void_p), ("dw", C.c_void_p)] + \
               [(k, C.c_int64) for k in ("n", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "pad", "ldx", "ldg", "out_oihw")] + \
               [("pre_x", C.c_void_p)] + [(k, C.c_int64) for k in ("rowrun_stride", "in_H", "in_W", "row0", "col0")]


class SgdParam(C.Structure):
    """nw_sgd_param (include/nwhead_hip.h)."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("momentum_buf", C.c_void_p), ("n", C.c_int64)]


class FwdOpts(C.Structure):
    """nw_fwd_opts (include/nwhead_hip.h): the options of ONE forward call."""
    _fields_ = [("struct_size", C.c_uint32), ("persistent_wgs", C.c_int32), ("force_split", C.c_int32),
                ("operand_form", C.c_int32), ("tables", C.c_void_p), ("tables_bytes", C.c_size_t),
                ("tables_sy", C.c_void_p), ("tables_N", C.c_int64)]


class FwdPlan(C.Structure):
    """nw_fwd_plan (include/nwhead_hip.h): the launch decision of the fused head for one call."""
    _fields_ = [(k, C.c_int32) for k in ("status", "rs", "bs", "n_stiles", "n_qtiles", "grid", "mode", "out", "dma", "persistent",
                                         "variant", "workgroups", "qgroup", "split_queries", "run_tables", "reserved")] + \
               [("lds_bytes", C.c_uint64)]


FORMS = {"fp32": 0, "split": 1, "half": 2}
OUTPUTS = {"log_probs": 0, "scores": 1, "candidates": 2}


def fwd_plan(B, N, d, C_, form="split", outputs="log_probs", k=0, norms=True, kind="euclidean", persistent_wgs=0, cus=0):
    """The library's launch decision for one forward call (nw_debug_fwd_plan): no launch, no device needed."""
    p = FwdPlan()
    check(load().nw_debug_fwd_plan(B, N, d, C_, FORMS[form], OUTPUTS[outputs], k, int(norms), SCORE_KINDS[kind],
                                   persistent_wgs, cus, C.byref(p)), "nw_debug_fwd_plan")
    return p


FWD_AREAS = ("main", "q_rows", "q_scale", "q_norm2", "lse", "slices")


class FwdLayout(C.Structure):
    """nw_fwd_layout (include/nwhead_hip.h): offset and size of the forward workspace's areas, in FWD_AREAS order."""
    _fields_ = [("off", C.c_uint64 * len(FWD_AREAS)), ("bytes", C.c_uint64 * len(FWD_AREAS)), ("total", C.c_uint64),
                ("n_slices", C.c_int32), ("reserved", C.c_int32)]


def fwd_layout(B, N, d, C_):
    """The library's map of the forward workspace for one shape (nw_debug_fwd_layout): no launch, no device needed."""
    m = FwdLayout()
    check(load().nw_debug_fwd_layout(B, N, d, C_, C.byref(m)), "nw_debug_fwd_layout")
    return m


BWD_ROUTES = ("valu", "mfma", "split")
BWD_AREAS = ("A", "Rs", "rq", "gls", "qn2", "sn2", "rs", "s_split", "s_scale", "q_split", "ascale", "qv", "gfac", "part", "part2")


class BwdPlan(C.Structure):
    """nw_bwd_plan (include/nwhead_hip.h): route, launch sizes and workspace map of the head's backward; `route` indexes
    BWD_ROUTES, `off` / `bytes` are in BWD_AREAS order."""
    _fields_ = [(k, C.c_int32) for k in ("status", "route", "coeff_threads", "parts_shared", "gq_chunks", "gq_k_chunk",
                                         "gs_chunks", "gs_k_chunk")] + \
               [("ld", C.c_int64), ("Bpad", C.c_int64), ("coeff_lds_bytes", C.c_uint64),
                ("off", C.c_uint64 * len(BWD_AREAS)), ("bytes", C.c_uint64 * len(BWD_AREAS)), ("total", C.c_uint64)]


def bwd_plan(B, N, d, C_, sup=0):
    """The library's plan of the backward for one shape under the current knobs (nw_debug_bwd_plan): no launch, no device."""
    p = BwdPlan()
    check(load().nw_debug_bwd_plan(B, N, d, C_, int(sup), C.byref(p)), "nw_debug_bwd_plan")
    return p


# Environment switches of the Python layer (the C library never reads the environment).  NW_SPLIT_ALWAYS travels in every
# forward call's nw_fwd_opts; the others are diagnostic knobs, forwarded once at load time (and again by sync_knobs()).
KNOBS = ("pvar", "qg", "tile_rs", "no_persistent", "split_queries", "bwd_no_mfma", "bwd_split",
         "xgemm_wgs", "split_lbits", "conv_max_wgs", "conv_skip_cfgs", "conv_force_cfg")
_KNOB_UNSET = -2 ** 31
_knob_state = {}


def sync_knobs():
    """Forward the NW_<KNOB> environment variables to the library's diagnostic knobs (nw_debug_set)."""
    if _lib is None:
        return
    for k in KNOBS:
        v = os.environ.get("NW_" + k.upper())
        val = _KNOB_UNSET if v is None or v == "" else int(v)
        if _knob_state.get(k, _KNOB_UNSET) != val:
            _lib.nw_debug_set(k.encode(), val)
            _knob_state[k] = val


def force_split():
    return os.environ.get("NW_SPLIT_ALWAYS", "") == "1"


def fwd_opts(tables=None, tables_bytes=0, persistent_wgs=0, tables_sy=None, tables_n=-1, operand_form=0):
    """An nw_fwd_opts for one forward call (a ctypes object: keep it alive across the call).  operand_form: 0 = the call's
    s_split holds split rows, 1 = half-precision rows (nw_pack_rows_f16)."""
    return FwdOpts(C.sizeof(FwdOpts), int(persistent_wgs), int(force_split()), int(operand_form), tables, int(tables_bytes),
                   tables_sy, int(tables_n))


def check(status: int, what: str):
    if status != 0:
        msg = load().nw_status_string(status).decode()
        raise NWHipError(f"{what}: {msg} (status {status})")
