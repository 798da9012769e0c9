"""ctypes binding of libcdc_hip.so (include/cdc_hip.h).  There is NO CPU fallback: if the HIP
library is missing or cannot be loaded, importing the product path fails loudly."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CDC_HIP_LIB selects another build of the same HIP library (A/B kernel experiments, tools/build_variant.sh)
LIB_PATH = os.environ.get("CDC_HIP_LIB") or os.path.join(_HERE, "libcdc_hip.so")

CDC_MEM_HOST, CDC_MEM_DEVICE = 0, 1
CDC_PRED_X, CDC_PRED_NOISE, CDC_PRED_NOISE_XTREE, CDC_PRED_V = 0, 1, 2, 3
CDC_CLIP_NONE, CDC_CLIP_ALL, CDC_CLIP_HALF = 0, 1, 2
CDC_MAX_LEVELS = 8
CDC_ELEM_F32, CDC_ELEM_U8 = 0, 1
CDC_FILL_EDGE, CDC_FILL_ZERO = 0, 1
CDC_METRIC_PSNR, CDC_METRIC_MSSSIM = 1, 2
CDC_TRACE_X0, CDC_TRACE_XT, CDC_TRACE_U8 = 1, 2, 4

_f = ctypes.POINTER(ctypes.c_float)
_i = ctypes.c_int
_vp = ctypes.c_void_p


class UnetConfig(ctypes.Structure):
    _fields_ = [("dim", ctypes.c_int32), ("channels", ctypes.c_int32),
                ("context_channels", ctypes.c_int32), ("out_dim", ctypes.c_int32),
                ("n_dim_mults", ctypes.c_int32), ("dim_mults", ctypes.c_int32 * CDC_MAX_LEVELS),
                ("n_context_dim_mults", ctypes.c_int32),
                ("context_dim_mults", ctypes.c_int32 * CDC_MAX_LEVELS)]


class CtxdecConfig(ctypes.Structure):
    _fields_ = [("dim", ctypes.c_int32), ("n_rev_mults", ctypes.c_int32),
                ("rev_mults", ctypes.c_int32 * CDC_MAX_LEVELS), ("out_channels", ctypes.c_int32),
                ("up_index", ctypes.c_int32)]


class HyperdecConfig(ctypes.Structure):
    _fields_ = [("n_layers", ctypes.c_int32), ("dims", ctypes.c_int32 * (CDC_MAX_LEVELS + 1))]


class EncoderConfig(ctypes.Structure):
    _fields_ = [("dim", ctypes.c_int32), ("channels", ctypes.c_int32), ("n_dim_mults", ctypes.c_int32),
                ("dim_mults", ctypes.c_int32 * CDC_MAX_LEVELS), ("n_hyper_mults", ctypes.c_int32),
                ("hyper_mults", ctypes.c_int32 * CDC_MAX_LEVELS), ("down_index", ctypes.c_int32)]


class ImageView(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("elem_kind", ctypes.c_int), ("Hf", ctypes.c_int), ("Wf", ctypes.c_int),
                ("as_saved", ctypes.c_int)]


class StreamInfo(ctypes.Structure):
    """cdc_stream_info of include/cdc_hip.h (cdc_entropy_peek_partial)."""
    _fields_ = [("hh", ctypes.c_int), ("wh", ctypes.c_int), ("arith", ctypes.c_int), ("has_rate", ctypes.c_int), ("rate", ctypes.c_float),
                ("has_size", ctypes.c_int), ("img_h", ctypes.c_int), ("img_w", ctypes.c_int), ("seg", ctypes.c_int), ("ny", ctypes.c_int),
                ("nx", ctypes.c_int), ("cg", ctypes.c_int), ("ng", ctypes.c_int), ("complete", ctypes.c_int),
                ("declared", ctypes.c_ulonglong), ("floor", ctypes.c_ulonglong)]


class ParallelInfo(ctypes.Structure):
    """cdc_parallel_info of include/cdc_hip.h (cdc_decode_parallel)."""
    _fields_ = [("sweeps", ctypes.c_int), ("rows_evaluated", ctypes.c_int), ("max_stride", ctypes.c_int), ("max_residual", ctypes.c_double)]


SEG_OK, SEG_ABSENT, SEG_DAMAGED = 0, 1, 2                       # CDC_SEG_* of include/cdc_hip.h


class CdcError(RuntimeError):
    pass


def build(force=False):
    """Compile libcdc_hip.so for gfx950 with hipcc (csrc/Makefile)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return LIB_PATH


def kernel_source_hash():
    """sha256[:16] over the HIP sources of the library (csrc/*.hip, *.h in name order): names the build a counter file was
    collected on (profiles/pmc_*_traffic.json carries it; bench.py quotes such a file only for the same kernels)."""
    import hashlib
    d = os.path.join(_HERE, "csrc")
    hsh = hashlib.sha256()
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):
            hsh.update(f.encode())
            hsh.update(open(os.path.join(d, f), "rb").read())
    return hsh.hexdigest()[:16]


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CdcError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
                       "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    try:
        import torch  # noqa: F401  (share torch's libamdhip64.so.7 so device pointers are compatible)
    except Exception:
        pass
    L = ctypes.CDLL(LIB_PATH)
    H = _vp
    pp = ctypes.POINTER(_vp)
    L.cdc_create.argtypes = [ctypes.POINTER(UnetConfig), _i, ctypes.POINTER(H)]
    L.cdc_destroy.argtypes = [H]
    L.cdc_destroy.restype = None
    L.cdc_last_error.argtypes = [H]
    L.cdc_last_error.restype = ctypes.c_char_p
    L.cdc_version.restype = ctypes.c_char_p
    L.cdc_set_arith.argtypes = [H, _i]
    L.cdc_get_arith.argtypes = [H]
    L.cdc_get_range_faults.argtypes = [H]
    L.cdc_get_nonfinite_results.argtypes = [H]
    L.cdc_num_tensors.argtypes = [H]
    L.cdc_tensor_info.argtypes = [H, _i, ctypes.POINTER(ctypes.c_char_p),
                                  ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(_i)]
    L.cdc_load_tensor.argtypes = [H, ctypes.c_char_p, _vp, ctypes.POINTER(ctypes.c_int64), _i]
    L.cdc_finalize_weights.argtypes = [H]
    L.cdc_unet_forward.argtypes = [H, _vp, _vp, pp, _i, _vp, _i, _i, _i, _i, _vp]
    L.cdc_unet_tap.argtypes = [H, ctypes.c_char_p, _vp, ctypes.POINTER(ctypes.c_int64)]
    L.cdc_ctxdec_create.argtypes = [ctypes.POINTER(CtxdecConfig), _i, ctypes.POINTER(H)]
    L.cdc_ctxdec_decode.argtypes = [H, _vp, pp, _i, _i, _i, _i, _i, _vp]
    L.cdc_encoder_create.argtypes = [ctypes.POINTER(EncoderConfig), _i, ctypes.POINTER(H)]
    L.cdc_simple_ctxdec_create.argtypes = [ctypes.POINTER(CtxdecConfig), _i, ctypes.POINTER(H)]
    L.cdc_simple_encoder_create.argtypes = [ctypes.POINTER(EncoderConfig), _i, ctypes.POINTER(H)]
    L.cdc_op_gdn.argtypes = [H, _vp, _vp, _vp, _vp, _i, _i, _i, _i]
    L.cdc_op_gdn_workgroups.argtypes = [H, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]
    L.cdc_encoder_encode.argtypes = [H, _vp, _vp, _vp, _i, _i, _i, _i, _vp]
    L.cdc_hyperdec_create.argtypes = [ctypes.POINTER(HyperdecConfig), _i, ctypes.POINTER(H)]
    L.cdc_hyperdec_decode.argtypes = [H, _vp, _vp, _vp, _i, _i, _i, ctypes.c_float, _i, _vp]
    L.cdc_entropy_encode.argtypes = [H, _vp, _vp, _vp, _i, _i, _i, _vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), _i, _vp]
    L.cdc_entropy_peek.argtypes = [_vp, ctypes.c_size_t, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)]
    L.cdc_entropy_set_limit.argtypes = [H, _i]
    L.cdc_entropy_decode.argtypes = [H, _vp, ctypes.POINTER(ctypes.c_size_t), _vp, _i, _vp, _vp, _i, _vp]
    L.cdc_enable_vbr.argtypes = [H]
    L.cdc_set_bitrate_scale.argtypes = [H, _vp, _i]
    L.cdc_entropy_peek_bitrate_scale.argtypes = [_vp, ctypes.c_size_t, ctypes.POINTER(_i), ctypes.POINTER(ctypes.c_float)]
    L.cdc_padded_size.argtypes = [H, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]
    L.cdc_frame_pad.argtypes = [H, _vp, _vp] + [_i] * 8 + [_vp]
    L.cdc_frame_crop.argtypes = [H, _vp, _vp] + [_i] * 7 + [_vp]
    L.cdc_entropy_set_image_scale.argtypes = [H, _i]
    L.cdc_entropy_encode_image.argtypes = [H, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), _i, _vp]
    L.cdc_entropy_peek_image_size.argtypes = [_vp, ctypes.c_size_t, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)]
    L.cdc_entropy_set_segments.argtypes = [H, _i]
    L.cdc_entropy_peek_segments.argtypes = [_vp, ctypes.c_size_t, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)]
    L.cdc_entropy_decode_window.argtypes = [H, _vp, ctypes.POINTER(ctypes.c_size_t), _vp, _i, ctypes.POINTER(ctypes.c_int32), _vp, _vp,
                                            ctypes.POINTER(_i), _i, _vp]
    L.cdc_entropy_set_hyper_groups.argtypes = [H, _i]
    L.cdc_entropy_peek_hyper_groups.argtypes = [_vp, ctypes.c_size_t, ctypes.POINTER(_i), ctypes.POINTER(_i)]
    L.cdc_entropy_peek_partial.argtypes = [_vp, ctypes.c_size_t, ctypes.POINTER(StreamInfo)]
    L.cdc_entropy_decode_partial.argtypes = [H, _vp, ctypes.POINTER(ctypes.c_size_t), _vp, _i, ctypes.POINTER(ctypes.c_int32), _vp, _vp, _vp, _i, _vp]
    L.cdc_segment_mask.argtypes = [H, _vp] + [_i] * 7 + [_vp, _i, _i, _vp]
    f64p = ctypes.POINTER(ctypes.c_double)
    L.cdc_distortion.argtypes = [H, ctypes.POINTER(ImageView), ctypes.POINTER(ImageView), _i, _i, _i, _i, f64p, f64p, f64p, _i, _vp]
    L.cdc_rate_map.argtypes = [H] + [_vp] * 9 + [_i, _i, _i, _i, _vp]
    L.cdc_distortion_map.argtypes = [H, ctypes.POINTER(ImageView), ctypes.POINTER(ImageView)] + [_i] * 6 + [_vp, _vp, _i, _vp]
    L.cdc_set_rdo.argtypes = [H, _vp, _i]
    L.cdc_entropy_rate_sweep.argtypes = [H, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _vp]
    L.cdc_op_rdo_quantize.argtypes = [H, _vp, _vp, _vp, _vp, _vp, _vp, _i, ctypes.c_longlong, _i, _vp]
    L.cdc_price_cells.argtypes = [H, _vp] + [_i] * 9 + [_vp, _i, _vp]
    L.cdc_set_rdo_map.argtypes = [H, _vp, _i, _i, _i, _i, _vp]
    L.cdc_op_rdo_quantize_map.argtypes = [H, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp]
    L.cdc_lpips_create.argtypes = [_i, ctypes.POINTER(H)]
    L.cdc_lpips.argtypes = [H, ctypes.POINTER(ImageView), ctypes.POINTER(ImageView), _i, _i, _i, f64p, f64p, _i, _vp]
    L.cdc_dequantize.argtypes = [H, _vp, _vp, _vp, ctypes.c_longlong, _i, _vp]
    L.cdc_bpp.argtypes = [H, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]
    L.cdc_set_schedule.argtypes = [H, _i, _vp, _vp, _vp, _vp, _vp, _vp]
    L.cdc_set_schedule_v.argtypes = [H, _i, _vp, _vp]
    L.cdc_ddim_step.argtypes = [H, _vp, _i, pp, _i, _vp, ctypes.c_float, _vp, _i, _i, _i, _i, _i,
                                _i, _vp]
    L.cdc_decode.argtypes = [H, _vp, pp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp]
    u64p = ctypes.POINTER(ctypes.c_uint64)
    L.cdc_decode_seeded.argtypes = [H, _vp, ctypes.c_float, u64p, ctypes.c_float, pp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp]
    L.cdc_set_solver.argtypes = [H, _i, _vp, _vp, _vp]
    L.cdc_decode_solver.argtypes = [H, _vp, ctypes.c_float, u64p, pp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp]
    L.cdc_solver_step.argtypes = [H, _vp, _vp, _i, pp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]
    L.cdc_op_solver_update.argtypes = [H, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]
    L.cdc_op_ddim_update.argtypes = [H, _vp, _vp, _vp, u64p, ctypes.c_float, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp]
    ip = ctypes.POINTER(_i)
    L.cdc_set_trace.argtypes = [H, ip, _i, _i, _i, _i]
    L.cdc_trace_info.argtypes = [H, ip, ip, ip, ip, ip, ip]
    L.cdc_trace_read.argtypes = [H, _i, _i, _i, _vp, _i, _vp]
    L.cdc_op_trace_tap.argtypes = [H, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp]
    L.cdc_repeat_images.argtypes =[H, _vp, _vp, _i, _i, ctypes.c_int64, _i, _i, _vp]
    L.cdc_decode_samples.argtypes = [H, ctypes.c_float, u64p, ctypes.c_float, pp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]
    L.cdc_decode_parallel.argtypes = [H, _vp, ctypes.c_float, u64p, ctypes.c_float, pp, _i, _vp, _i, _i, _i, _i, _i, _i, ctypes.c_float,
                                      ctypes.POINTER(_i), ctypes.POINTER(ParallelInfo), _i, _vp]
    L.cdc_parallel_stride.argtypes = [ctypes.POINTER(ctypes.c_double), _i, _i, _i, ctypes.c_double, ctypes.c_double]
    L.cdc_parallel_row_steps.argtypes = [_i, _i, _i, ctypes.POINTER(_i)]
    L.cdc_op_window_update.argtypes = [H, _vp, _vp, u64p, ctypes.c_float, _i, _i, ctypes.POINTER(ctypes.c_double)] + [_i] * 7 + [_vp]
    L.cdc_sample_moments.argtypes = [H, _vp, _i, _i, ctypes.c_int64, _i, _vp, _vp, _i, _i, _vp]
    L.cdc_sample_select.argtypes = [H, _vp, ctypes.POINTER(_i), _vp, _i, _i, ctypes.c_int64, _i, _vp]
    L.cdc_randn.argtypes = [H, u64p, _i, ctypes.c_int64, ctypes.c_uint32, ctypes.c_float, _vp, _i, _vp]
    L.cdc_randn_host.argtypes = [u64p, _i, ctypes.c_int64, ctypes.c_uint32, ctypes.c_float, _vp]
    L.cdc_philox4x32_10.argtypes = [ctypes.POINTER(ctypes.c_uint32)] * 3
    i32p = ctypes.POINTER(ctypes.c_int32)
    L.cdc_set_noise_frames.argtypes = [H, i32p, _i]
    L.cdc_randn_framed.argtypes = [H, u64p, i32p, _i, _i, _i, _i, ctypes.c_uint32, ctypes.c_float, _vp, _i, _vp]
    L.cdc_randn_framed_host.argtypes = [u64p, i32p, _i, _i, _i, _i, ctypes.c_uint32, ctypes.c_float, _vp]
    L.cdc_tile_gather.argtypes = [H, _vp, _vp, i32p] + [_i] * 8 + [_vp]
    L.cdc_tile_blend.argtypes = [H, _vp, _vp, i32p, _i, i32p, _i, _vp] + [_i] * 14 + [_vp]
    L.cdc_prof_enable.argtypes = [H, _i]
    L.cdc_prof_name.argtypes = [_i]
    L.cdc_prof_name.restype = ctypes.c_char_p
    L.cdc_prof_get.argtypes = [H, _i, ctypes.POINTER(ctypes.c_double),
                               ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double),
                               ctypes.POINTER(ctypes.c_double)]
    L.cdc_prof_reset.argtypes = [H]
    L.cdc_set_decode_chains.argtypes = [H, _i]
    L.cdc_decode_chains.argtypes = [H, _i, _i, _i]
    L.cdc_prof_num_ops.argtypes = [H]
    L.cdc_prof_op.argtypes = [H, _i, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_double),
                              ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)]
    L.cdc_op_conv2d.argtypes = [H, _vp, _vp, _vp, _vp] + [_i] * 9 + [_vp, _vp, _i, _vp, _vp]
    L.cdc_op_conv_transpose2d.argtypes = [H, _vp, _vp, _vp, _vp] + [_i] * 5
    L.cdc_op_chan_layernorm.argtypes = [H, _vp, _vp, _vp, _vp, _i, _i, _i]
    L.cdc_op_chan_layernorm_ex.argtypes = [H, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i]
    L.cdc_op_ln_form.argtypes = [H, _i, _i, _i, _i, _i] + [ctypes.POINTER(_i)] * 4
    L.cdc_op_sum_slices.argtypes = [H, _vp, _i, _vp, _i, ctypes.c_longlong]
    L.cdc_op_linear_attention.argtypes = [H] + [_vp] * 7 + [_i] * 4
    L.cdc_op_stress.argtypes = [H, _i]
    L.cdc_op_stress_result.argtypes = [H, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    L.cdc_probe_mfma_f16.argtypes = [_i, _i, _i, ctypes.POINTER(ctypes.c_double)]
    L.cdc_probe_hbm_copy.argtypes = [_i, ctypes.c_size_t, _i, ctypes.POINTER(ctypes.c_double)]
    _lib = L
    return L


EXPORTS = ["cdc_create", "cdc_destroy", "cdc_last_error", "cdc_version", "cdc_num_tensors",
           "cdc_tensor_info", "cdc_load_tensor", "cdc_finalize_weights", "cdc_unet_forward",
           "cdc_set_schedule", "cdc_ddim_step", "cdc_decode", "cdc_prof_enable",
           "cdc_prof_num_classes", "cdc_prof_name", "cdc_prof_get", "cdc_prof_reset",
           "cdc_op_conv2d", "cdc_op_conv_transpose2d", "cdc_op_chan_layernorm",
           "cdc_op_linear_attention", "cdc_ctxdec_create", "cdc_ctxdec_decode", "cdc_hyperdec_create",
           "cdc_hyperdec_decode", "cdc_dequantize", "cdc_bpp", "cdc_encoder_create",
           "cdc_encoder_encode", "cdc_set_arith", "cdc_get_arith", "cdc_unet_tap", "cdc_prof_num_ops", "cdc_prof_op",
           "cdc_entropy_encode", "cdc_entropy_peek", "cdc_entropy_set_limit", "cdc_entropy_decode", "cdc_get_range_faults",
           "cdc_get_nonfinite_results", "cdc_set_schedule_v", "cdc_probe_mfma_f16", "cdc_probe_hbm_copy",
           "cdc_op_stress", "cdc_op_stress_result", "cdc_enable_vbr", "cdc_set_bitrate_scale", "cdc_entropy_peek_bitrate_scale",
           "cdc_padded_size", "cdc_frame_pad", "cdc_frame_crop", "cdc_entropy_set_image_scale", "cdc_entropy_encode_image",
           "cdc_entropy_peek_image_size", "cdc_decode_seeded", "cdc_randn", "cdc_randn_host", "cdc_philox4x32_10",
           "cdc_distortion", "cdc_lpips_create", "cdc_lpips", "cdc_simple_encoder_create", "cdc_simple_ctxdec_create", "cdc_op_gdn",
           "cdc_op_gdn_workgroups", "cdc_op_chan_layernorm_ex", "cdc_op_ln_form", "cdc_op_sum_slices",
           "cdc_set_solver", "cdc_decode_solver", "cdc_solver_step", "cdc_op_solver_update", "cdc_op_ddim_update",
           "cdc_repeat_images", "cdc_decode_samples", "cdc_sample_moments", "cdc_sample_select",
           "cdc_set_trace", "cdc_trace_info", "cdc_trace_read", "cdc_op_trace_tap",
           "cdc_rate_map", "cdc_distortion_map", "cdc_set_rdo", "cdc_entropy_rate_sweep", "cdc_op_rdo_quantize",
           "cdc_price_cells", "cdc_set_rdo_map", "cdc_op_rdo_quantize_map",
           "cdc_set_noise_frames", "cdc_randn_framed", "cdc_randn_framed_host", "cdc_tile_gather", "cdc_tile_blend",
           "cdc_entropy_set_segments", "cdc_entropy_peek_segments", "cdc_entropy_decode_window",
           "cdc_entropy_set_hyper_groups", "cdc_entropy_peek_hyper_groups",
           "cdc_entropy_peek_partial", "cdc_entropy_decode_partial", "cdc_segment_mask",
           "cdc_set_decode_chains", "cdc_decode_chains", "cdc_decode_parallel", "cdc_op_window_update", "cdc_parallel_stride",
           "cdc_parallel_row_steps"]


def handle_status(handle):
    """{'arith', 'range_faults', 'nonfinite_results'} of one library handle (None -> zeros): the fp16-range guard of
    include/cdc_hip.h repeats a call in the full-range arithmetic and LEAVES the handle there -- these tell."""
    if handle is None:
        return {"arith": None, "range_faults": 0, "nonfinite_results": 0}
    L = lib()
    return {"arith": int(L.cdc_get_arith(handle)), "range_faults": int(L.cdc_get_range_faults(handle)),
            "nonfinite_results": int(L.cdc_get_nonfinite_results(handle))}


def check(handle, rc):
    if rc != 0:
        msg = lib().cdc_last_error(handle)
        msg = msg.decode() if msg else ""
        if "must be multiples of" in msg:
            msg += " -- padded_size(H, W) gives the frame; compress() / decompress() / the compressor's forward() pad any size themselves"
        raise CdcError(f"libcdc_hip error {rc}: {msg}")


def device_index_of(device):
    """The device index a model's `device=` / `.to()` argument names: an int, "cuda", "cuda:3", torch.device("cuda", 2); 0 when it
    names none (None, "cuda", an object whose .index is None)."""
    if device is None:
        return 0
    if isinstance(device, str):
        return int(device.split(":")[1]) if ":" in device else 0
    if hasattr(device, "index"):
        return int(device.index or 0)
    return int(device)


class Handle:
    """The one owner of a library handle (cdc_handle*) of the Python mirror: created on first use, destroyed with this object, and
    re-created on another device with everything it was given.

    create: the constructor's name ("cdc_create", "cdc_ctxdec_create", ...); config: a callable returning its filled config structure
    (None: the constructor takes none, cdc_lpips_create); setup(ptr): runs after every creation (cdc_enable_vbr, ...) -- when it raises,
    the fresh handle is destroyed and the next use tries again."""

    def __init__(self, create, config, device_index, setup=None):
        self.create, self.config, self.device_index, self.setup = create, config, int(device_index), setup
        self.raw = None            # the c_void_p while a handle exists
        self.tensors = {}          # name -> a float32 copy of the array load() was given, in its shape (what a move replays)
        self.finalized = False     # finalize() has run since the last load()

    @property
    def ptr(self):
        """The handle; a new one gets setup(), every remembered tensor, and final weights again if they were final."""
        if self.raw is None:
            L = lib()
            h = _vp()
            args = () if self.config is None else (ctypes.byref(self.config()),)
            rc = getattr(L, self.create)(*args, self.device_index, ctypes.byref(h))
            if rc != 0:
                raise CdcError(f"{self.create} failed ({rc}): {L.cdc_last_error(None).decode()}")
            self.raw = h
            try:
                if self.setup is not None:
                    self.setup(h)
                for name, a in self.tensors.items():
                    self._load(h, name, a)
                if self.finalized:
                    check(h, L.cdc_finalize_weights(h))
            except BaseException:
                self.close()
                raise
        return self.raw

    def manifest(self):
        """[(name, shape)] of the required tensors, in the library's (= the reference state_dict's) order."""
        L, h = lib(), self.ptr
        out = []
        for i in range(L.cdc_num_tensors(h)):
            name = ctypes.c_char_p()
            shape = (ctypes.c_int64 * 4)()
            nd = ctypes.c_int()
            check(h, L.cdc_tensor_info(h, i, ctypes.byref(name), shape, ctypes.byref(nd)))
            out.append((name.value.decode(), tuple(shape[j] for j in range(nd.value))))
        return out

    @staticmethod
    def _load(h, name, a):
        shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
        check(h, lib().cdc_load_tensor(h, name.encode(), a.ctypes.data, shape, a.ndim))

    def load(self, name, array):
        a = np.array(array, dtype=np.float32, order="C")       # a copy: what a move replays is what was loaded, whatever the caller does next
        self._load(self.ptr, name, a)
        self.tensors[name] = a
        self.finalized = False

    def finalize(self):
        h = self.ptr
        check(h, lib().cdc_finalize_weights(h))
        self.finalized = True

    def status(self):
        return handle_status(self.raw)

    def close(self):
        if self.raw is not None:
            h, self.raw = self.raw, None
            lib().cdc_destroy(h)

    def move(self, device_index):
        """Bind to another device: the handle goes, what was loaded stays; the next `ptr` creates it there.  Touches no device."""
        if int(device_index) != self.device_index:
            self.close()
            self.device_index = int(device_index)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
