"""ctypes binding of libkair_hip.so (include/kair_hip.h).

This is the ONLY way the product reaches its kernels.  There is no CPU or PyTorch fallback: if the
library is missing or a call fails, a RuntimeError is raised (tests/test_boundary.py checks both).
Tensors are passed as raw device pointers; the current torch stream is passed explicitly.
"""
import ctypes
import os

import torch

# KAIR_LIB=debug: the debug-ablation build (python -m kair_amd.build --debug-ablations), for the
# perf-investigation tools only; the release library is the default and the only one tests / bench use
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                        {"debug": "libkair_hip_dbg.so", "base": "libkair_hip_base.so"}.get(os.environ.get("KAIR_LIB"),
                                                                                          "libkair_hip.so"))
# KAIR_LIB=base: an A/B baseline library (same ABI, earlier sources) placed there by hand; never shipped

F32, BF16, F16 = 0, 1, 3
X3 = 2   # KAIR_COMPUTE_X3: split-fp16 arithmetic (hi.hi + hi.lo + lo.hi of power-of-2-scaled fp16 pairs)
X3_WEXP = 12   # KAIR_X3_WEXP: the exponent of the fp16 weight packs
LD_ROWS, LD_IM2COL3, LD_QKVBLK, LD_S2D = 0, 1, 2, 3
USR_SRC_NCHW, USR_SRC_PSF, USR_SRC_ZUP, USR_SRC_NHWC = 0, 1, 2, 3
USR_COL_FB, USR_COL_FBFY, USR_COL_DATA_FWD, USR_COL_DATA_BWD = 0, 1, 2, 3
USR_CHAN_CHUNKS = 64
USR_PAD_REPLICATE, USR_PAD_ZERO, USR_PAD_FOLD, USR_CROP_NCHW = 0, 1, 2, 3
OUT_ROWS, OUT_QKVBLK, OUT_PSHUF, OUT_PUNSHUF, OUT_NCHW, OUT_PSHUF_NCHW = 0, 1, 2, 3, 4, 5
OUT_PSHUF_SPM, OUT_PUNSHUF_SPM = 6, 7
ACT_NONE, ACT_GELU, ACT_LEAKY, ACT_RELU = 0, 1, 2, 3

c_long, c_int, c_float, c_vp = ctypes.c_long, ctypes.c_int, ctypes.c_float, ctypes.c_void_p


class Operand(ctypes.Structure):
    _fields_ = [("ptr", c_vp), ("dtype", c_int), ("mode", c_int), ("ld", c_long),
                ("win_H", c_int), ("win_W", c_int), ("win_ws", c_int), ("win_shift", c_int),
                ("im_H", c_int), ("im_W", c_int), ("im_C", c_int), ("im_flip", c_int),
                ("qkv_nh", c_int), ("qkv_hdp", c_int), ("qkv_tok", c_int),
                ("rowscale", c_vp), ("rows_per_scale", c_int), ("ones_col", c_int), ("ones_in_data", c_int),
                ("im_up", c_int), ("w_split", c_int), ("a_split", c_int), ("lo_ptr", c_vp), ("x3_exp", c_int),
                ("im_dil", c_int)]


class CopyDesc(ctypes.Structure):
    _fields_ = [("out", c_vp), ("dtype", c_int), ("ld", c_long), ("rowscale", c_vp), ("rows_per_scale", c_int),
                ("win_H", c_int), ("win_W", c_int), ("win_ws", c_int), ("win_shift", c_int), ("out_lo", c_vp),
                ("x3_exp", c_int)]


def copy_desc(out, ld=None, rowscale=None, rows_per_scale=1, win=None, x3_exp=0):
    """Row-scaled cast copy target (GEMM A operand); win puts the rows in Swin window order.  out an fp16 pair
    [2, ...] (hi plane, lo plane): the x3 pair of v 2^x3_exp."""
    d = CopyDesc()
    d._keep = (out, rowscale)
    if out.dtype == torch.float16:
        d.out, d.out_lo, d.dtype, d.x3_exp = ptr(out[0]), ptr(out[1]), F16, int(x3_exp)
    else:
        d.out, d.dtype = ptr(out), dtype_code(out)
    d.ld = ld if ld is not None else out.shape[-1]
    d.rowscale, d.rows_per_scale = ptr(rowscale), rows_per_scale
    if win:
        d.win_H, d.win_W, d.win_ws, d.win_shift = win
    return d


class Epilogue(ctypes.Structure):
    _fields_ = [("out", c_vp), ("out_dtype", c_int), ("out_mode", c_int), ("ldo", c_long),
                ("win_H", c_int), ("win_W", c_int), ("win_ws", c_int), ("win_shift", c_int),
                ("bias", c_vp), ("act", c_int), ("slope", c_float),
                ("out_pre", c_vp), ("pre_dtype", c_int), ("ldp", c_long),
                ("resid", c_vp), ("ldr", c_long),
                ("rowscale", c_vp), ("rows_per_scale", c_int),
                ("gate", c_vp), ("gate_dtype", c_int), ("ldg", c_long), ("gate_kind", c_int),
                ("ps_r", c_int), ("ps_H", c_int), ("ps_W", c_int),
                ("qkv_nh", c_int), ("qkv_hdp", c_int), ("qkv_tok", c_int),
                ("img_mean", c_vp), ("img_range", c_float), ("img_C", c_int), ("img_H", c_int), ("img_W", c_int),
                ("out_ones_col_p1", c_int), ("resid2", c_vp), ("ldr2", c_long), ("pre_kind", c_int),
                ("a_copy", c_vp), ("ld_acopy", c_long), ("acopy_ones_col_p1", c_int), ("out_lo", c_vp),
                ("x3_out_exp", c_int)]


class WMap(ctypes.Structure):
    _fields_ = [("kind", c_int), ("N", c_int), ("K", c_int), ("nG", c_int), ("nGr", c_int), ("nGp", c_int),
                ("kG", c_int), ("kGr", c_int), ("kGp", c_int), ("n_perm", c_int)]


class WgradJob(ctypes.Structure):
    _fields_ = [("A", Operand), ("B", Operand), ("N", c_int), ("K", c_int), ("map", WMap), ("grad", c_vp),
                ("bias_grad", c_vp), ("ones_col", c_int)]


class LnParamJob(ctypes.Structure):
    _fields_ = [("part", c_vp), ("nb", c_long), ("C", c_int), ("dgamma", c_vp), ("dbeta", c_vp), ("accumulate", c_int)]


class DtabJob(ctypes.Structure):
    _fields_ = [("ws", c_vp), ("nWin", c_long), ("nh", c_int), ("dtype", c_int), ("dtable", c_vp), ("accumulate", c_int),
                ("win_ws", c_int)]


class PackJob(ctypes.Structure):
    _fields_ = [("src", c_vp), ("dst", c_vp), ("dst_dtype", c_int), ("reserved", c_int), ("map", WMap),
                ("total", c_long)]


_SIGS = {
    "kair_gemm_nt": [ctypes.POINTER(Operand), ctypes.POINTER(Operand), ctypes.POINTER(Epilogue), c_long, c_int, c_int,
                     c_int, c_vp],
    "kair_wgrad_splits": [c_long, c_int, c_int],
    "kair_conv3x3_halo_geometry": [c_int, c_int, c_int, c_long, c_int],
    "kair_gemm_tn": [ctypes.POINTER(Operand), ctypes.POINTER(Operand), c_vp, c_int, c_long, c_int, c_int, c_int, c_vp],
    "kair_wgrad_grouped_ws": [ctypes.POINTER(WgradJob), c_int, c_long],
    "kair_wgrad_grouped": [ctypes.POINTER(WgradJob), c_int, c_long, c_vp, c_vp],
    "kair_wgrad_grouped_ex": [ctypes.POINTER(WgradJob), c_int, c_long, c_vp, c_int, c_vp],
    "kair_layernorm_bwd_blocks": [c_long],
    "kair_ln_param_reduce_grouped": [ctypes.POINTER(LnParamJob), c_int, c_vp],
    "kair_window_attn_bwd_groups": [c_long, c_int, c_int],
    "kair_attn_dtable_grouped": [ctypes.POINTER(DtabJob), c_int, c_vp],
    "kair_pack_weight": [c_vp, c_vp, c_int, ctypes.POINTER(WMap), c_vp],
    "kair_pack_table_bytes": [c_int],
    "kair_pack_table_build": [ctypes.POINTER(PackJob), c_int, c_vp],
    "kair_pack_weights": [c_vp, c_int, c_long, c_vp],
    "kair_wgrad_finalize": [c_vp, c_int, ctypes.POINTER(WMap), c_vp, c_vp, c_int, c_int, c_vp],
    "kair_colsum_ws": [c_int],
    "kair_colsum": [ctypes.POINTER(Operand), c_long, c_int, ctypes.POINTER(WMap), c_vp, c_vp, c_int, c_vp],
    "kair_layernorm_fwd": [c_vp, c_long, c_vp, c_int, c_long, c_vp, c_vp, c_vp, c_vp, c_long, c_int, c_float, c_int,
                           c_int, c_int, c_int, c_int, c_vp],
    "kair_layernorm_fwd_x3": [c_vp, c_long, c_vp, c_vp, c_long, c_vp, c_vp, c_vp, c_vp, c_long, c_int, c_float, c_int,
                              c_int, c_int, c_int, c_int, c_int, c_vp],
    "kair_layernorm_bwd": [c_vp, c_long, c_vp, c_int, c_long, c_vp, c_vp, c_vp, c_vp, c_long, c_int, c_vp, c_vp, c_int,
                           c_vp, c_long, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(CopyDesc), c_vp],
    "kair_row_copy": [c_vp, c_long, c_long, c_int, ctypes.POINTER(CopyDesc), c_vp],
    "kair_gemm_nt_x3_lnbwd": [ctypes.POINTER(Operand), ctypes.POINTER(Operand), c_long, c_int, c_int, c_int, c_int, c_int,
                              c_int, c_vp, c_long, c_vp, c_vp, c_vp, c_int, c_vp, c_long, c_vp, ctypes.POINTER(CopyDesc),
                              c_vp],
    "kair_gemm_nt_x3_lnbwd_parts": [c_long, c_int],
    "kair_window_attn_fwd": [c_vp, c_int, c_vp, c_vp, c_long, c_vp, c_long, c_int, c_int, c_float, c_int, c_int, c_int,
                             c_int, c_vp, c_int, c_vp],
    "kair_window_attn_bwd_ws": [c_long, c_int],
    "kair_window_attn_bwd_ws_w": [c_long, c_int, c_int],
    "kair_window_attn_fwd_w": [c_vp, c_int, c_vp, c_vp, c_long, c_vp, c_long, c_int, c_int, c_float, c_int, c_int, c_int,
                               c_int, c_vp, c_int, c_int, c_int, c_vp],
    "kair_window_attn_bwd_w": [c_vp, c_vp, c_long, c_vp, c_long, c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_long,
                               c_int, c_int, c_float, c_int, c_int, c_int, c_vp, c_int, c_int, c_int, c_vp],
    "kair_window_attn_fwd_x3_w": [c_vp, c_vp, c_vp, c_vp, c_vp, c_long, c_vp, c_long, c_int, c_int, c_float, c_int, c_int,
                                  c_int, c_int, c_int, c_int, c_int, c_vp],
    "kair_window_attn_bwd_x3_w": [c_vp, c_vp, c_vp, c_vp, c_long, c_vp, c_vp, c_long, c_vp, c_vp, c_vp, c_vp, c_vp, c_int,
                                  c_vp, c_long, c_int, c_int, c_float, c_int, c_int, c_int, c_int, c_int, c_int, c_vp],
    "kair_window_attn_bwd": [c_vp, c_vp, c_long, c_vp, c_long, c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_long, c_int,
                             c_int, c_float, c_int, c_int, c_int, c_vp, c_int, c_vp],
    "kair_window_attn_bwd_ex": [c_vp, c_vp, c_long, c_vp, c_long, c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_long,
                                c_int, c_int, c_float, c_int, c_int, c_int, c_vp, c_int, c_int, c_vp],
    "kair_window_attn_fwd_ex": [c_vp, c_int, c_vp, c_vp, c_long, c_vp, c_long, c_int, c_int, c_float, c_int, c_int, c_int,
                                c_int, c_vp, c_int, c_int, c_vp],
    "kair_image_to_nhwc": [c_vp, c_vp, c_int, c_int, c_vp, c_float, c_int, c_int, c_int, c_int, c_vp],
    "kair_image_to_nhwc_hilo": [c_vp, c_vp, c_int, c_vp, c_float, c_int, c_int, c_int, c_int, c_vp],
    "kair_ffd_pack": [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp],
    "kair_conv3x3_narrow_fwd": [c_vp, c_long, c_int, c_vp, c_vp, c_int, c_vp, c_float, c_vp, c_vp, c_int, c_int, c_int,
                                c_vp],
    "kair_conv3x3_wr_tile": [c_int, c_int, c_int, c_int, c_int, c_int],
    "kair_conv3x3_wr": [c_vp, c_int, c_long, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_long, c_vp, c_int, c_long, c_vp,
                        c_long, c_int, c_int, c_int, c_int, c_int, c_int, c_vp],
    "kair_conv3x3_wr_ex": [c_vp, c_int, c_long, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_long, c_vp, c_int, c_long, c_vp,
                           c_int, c_int, c_float, c_vp, c_long, c_vp, c_long, c_int, c_int, c_int, c_int, c_int, c_int,
                           c_vp],
    "kair_conv3x3_dil_ok": [c_int, c_int, c_int],
    "kair_conv3x3_dil": [c_vp, c_long, c_int, c_int, c_vp, c_int, c_vp, c_int, c_float, c_vp, c_int, c_long, c_int, c_int,
                         c_int, c_int, c_int, c_vp],
    "kair_conv3x3_wr_x3_tile": [c_int, c_int, c_int, c_int, c_int],
    "kair_conv3x3_wr_x3": [c_vp, c_long, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_long, c_vp, c_long, c_int, c_int, c_int,
                           c_int, c_int, c_vp],
    "kair_conv3x3_narrow_dgrad_ws": [],
    "kair_conv3x3_narrow_dgrad": [c_vp, c_long, c_vp, c_int, c_vp, c_vp, c_int, c_long, c_int, c_int, c_int, c_int, c_vp],
    "kair_conv3x3_narrow_wgrad_ws": [c_int],
    "kair_conv3x3_narrow_wgrad": [c_vp, c_long, c_vp, c_long, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp],
    "kair_conv3x3_narrow_x3_ws": [],
    "kair_conv3x3_narrow_fwd_x3": [c_vp, c_long, c_int, c_vp, c_vp, c_int, c_vp, c_vp, c_float, c_vp, c_vp, c_int, c_int,
                                   c_int, c_vp],
    "kair_conv3x3_narrow_dgrad_x3": [c_vp, c_long, c_int, c_vp, c_int, c_vp, c_vp, c_long, c_int, c_int, c_int, c_int,
                                     c_vp],
    "kair_conv3x3_narrow_wgrad_x3": [c_vp, c_long, c_int, c_vp, c_long, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_int,
                                     c_int, c_int, c_vp],
    "kair_l1_loss": [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_float, c_int, c_int, c_int, c_int, c_vp, c_vp],
    "kair_ssim_workspace_bytes": [c_int, c_int, c_int, c_int],
    "kair_ssim_loss": [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_float, c_int, c_int, c_int, c_int, c_vp, c_vp],
    "kair_ssim_loss_nchw": [c_vp, c_vp, c_vp, c_vp, c_float, c_int, c_int, c_int, c_int, c_vp, c_vp],
    "kair_image_metrics_workspace_bytes": [c_int, c_int, c_int, c_int, c_int, c_int],
    "kair_image_metrics": [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp],
    "kair_psnr_db": [c_vp, c_long, c_vp, c_long, c_int, ctypes.c_double, c_vp],
    "kair_psnr_db_ref": [ctypes.c_double, ctypes.c_double],
    "kair_charbonnier_loss": [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_float, c_float, c_int, c_int, c_int, c_int,
                              c_vp, c_vp],
    "kair_axpy": [c_vp, c_vp, c_float, c_long, c_vp],
    "kair_axpby": [c_vp, c_vp, c_float, c_float, c_long, c_vp],
    "kair_bn_ws": [c_int],
    "kair_bn_fwd": [c_vp, c_long, c_vp, c_int, c_long, c_long, c_int, c_vp, c_vp, c_vp, c_vp, c_float, c_float, c_int,
                    c_vp, c_vp, c_int, c_float, c_vp, c_vp],
    "kair_bn_bwd": [c_vp, c_long, c_vp, c_int, c_long, c_vp, c_long, c_vp, c_int, c_long, c_long, c_int, c_vp, c_vp, c_vp,
                    c_int, c_float, c_vp, c_vp, c_int, c_vp, c_vp],
    "kair_axpby_rows": [c_vp, c_long, c_vp, c_long, c_long, c_int, c_float, c_float, c_vp],
    "kair_act_grad_cast": [c_vp, c_long, c_vp, c_int, c_long, c_vp, c_int, c_long, c_long, c_int, c_int, c_float, c_float,
                           c_vp],
    "kair_sumpool2x": [c_vp, c_long, c_vp, c_long, c_int, c_int, c_int, c_int, c_int, c_vp],
    "kair_act_grad_punshuf": [c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_vp],
    "kair_synth_dpsr": [c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp,
                        c_int, ctypes.c_ulonglong, ctypes.c_ulonglong, c_vp, c_vp, c_vp],
    "kair_adam_ema": [c_vp, c_vp, c_vp, c_vp, c_vp, c_long, c_vp, c_float, c_float, c_float, c_float, c_float, c_vp],
    "kair_adam_ema_ex": [c_vp, c_vp, c_vp, c_vp, c_vp, c_long, c_vp, c_float, c_float, c_float, c_float, c_float, c_vp,
                         c_vp],
    "kair_l2_loss": [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_float, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp],
    "kair_grad_norm_ws": [ctypes.POINTER(c_int), ctypes.POINTER(c_int)],
    "kair_grad_norm": [c_vp, c_long, c_vp, c_vp, c_vp],
    "kair_adam_ema_clip": [c_vp, c_vp, c_vp, c_vp, c_vp, c_long, c_vp, c_float, c_float, c_float, c_float, c_float, c_vp,
                           c_vp, c_float, c_vp],
    "kair_range_check": [c_vp, c_vp, c_long, c_vp, c_float, c_vp, c_vp],
    "kair_gate_hold": [c_int, c_vp],
    "kair_gate_release": [],
    "kair_gate_status": [],
    "kair_ktime_begin": [c_int],
    "kair_ktime_count": [],
    "kair_ktime_end": [],
    "kair_ktime_read": [c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_char_p)],
    "kair_usr_fft_rows": [c_vp, c_int, c_int, c_long, c_int, c_int, c_int, c_vp, c_int, c_int, c_int, c_vp],
    "kair_usr_fft_cols": [c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int,
                          c_vp],
    "kair_usr_ifft_rows": [c_vp, c_vp, c_int, c_int, c_int, c_long, c_float, c_int, c_int, c_int, c_vp],
    "kair_usr_seg_sum": [c_vp, c_int, c_int, c_float, c_vp, c_int, c_int, c_vp],
    "kair_usr_chan_sum": [c_vp, c_long, c_int, c_long, c_int, c_vp, c_vp, c_int, c_int, c_vp],
    "kair_usr_upsample_nearest": [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp],
    "kair_usr_pack_input": [c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_long, c_vp],
    "kair_usr_pad": [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_vp],
    "kair_hypanet_fwd": [c_vp, c_float] + [c_vp] * 6 + [c_int, c_int, c_int, c_vp, c_vp],
    "kair_hypanet_bwd": [c_vp, c_float] + [c_vp] * 6 + [c_int, c_int, c_int, c_vp] + [c_vp] * 6 + [c_int, c_vp],
    "kair_synth_sr": [c_vp, c_int, c_int, c_int, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp,
                      c_vp],
    "kair_synth_dn": [c_vp, c_int, c_int, c_int, c_vp, c_int, c_int, c_float, ctypes.c_ulonglong, ctypes.c_ulonglong,
                      c_vp, c_vp, c_vp],
    "kair_synth_dn_map": [c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_int, c_int, c_int, ctypes.c_ulonglong,
                          ctypes.c_ulonglong, c_vp, c_vp, c_vp],
    "kair_synth_dn_level": [c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_int, c_int, c_int, ctypes.c_ulonglong,
                            ctypes.c_ulonglong, c_vp, c_vp, c_vp, c_vp],
    "kair_usr_gauss_kernels": [c_vp, c_int, c_vp, c_int, c_vp, c_int, c_int, c_int, c_vp, c_vp],
    "kair_synth_usr": [c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_int, c_vp,
                       c_int, c_int, ctypes.c_ulonglong, ctypes.c_ulonglong, c_vp, c_vp, c_int, c_vp],
    "kair_usr_degrade": [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_long, c_int, c_int, c_vp, c_int, c_int,
                         ctypes.c_ulonglong, ctypes.c_ulonglong, c_vp, c_int, c_vp],
    "kair_srmd_kernels": [c_vp, c_int, c_vp, c_int, c_int, c_vp, c_vp, c_vp],
    "kair_synth_srmd": [c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_int, c_int,
                        c_vp, c_vp, c_int, ctypes.c_ulonglong, ctypes.c_ulonglong, c_vp, c_vp, c_vp],
    "kair_jpeg_workspace_bytes": [c_int, c_int, c_int, c_int],
    "kair_jpeg_roundtrip": [c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_vp],
    "kair_rgb2gray8": [c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp],
    "kair_synth_jpeg": [c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp],
    "kair_bsr_crop": [c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_int, c_int, c_vp, c_vp],
    "kair_bsr_finish": [c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp],
    "kair_bsr_kernels": [c_vp, c_int, c_int, c_int, c_int, c_vp, c_long, c_vp],
    "kair_bsr_ops": [c_vp, c_vp, c_int, c_int, c_int, c_vp, c_int, c_vp, c_long, c_vp, c_vp, c_vp, c_vp, c_int, c_int,
                     c_int, ctypes.c_ulonglong, ctypes.c_ulonglong, c_int, c_int, c_vp],
    "kair_jpeg_roundtrip_var": [c_vp, c_int, c_int, c_int, c_vp, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_vp],
    "kair_swin_attn_fwd": [c_vp, c_long, c_vp, c_vp, c_float, c_int, c_vp, c_long, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                           c_float, c_vp, c_long, c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_long, c_long, c_int,
                           c_int, c_int, c_int, c_int, c_vp],
    "kair_swin_mlp_fwd": [c_vp, c_long, c_vp, c_vp, c_float, c_int, c_vp, c_long, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                          c_long, c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_long, c_long, c_int, c_int, c_int, c_vp],
    "kair_debug_attn_stamps": [c_vp, c_int],
    "kair_debug_fused_stamps": [c_vp, c_int],
    "kair_debug_x3_stamps": [c_vp, c_int],
    "kair_swin_mlp_bwd_ws": [],
    "kair_swin_mlp_bwd": [c_vp, c_long, c_vp, c_long, c_vp, c_vp, c_vp, c_long, c_vp, c_long, c_vp, c_vp, c_vp, c_int,
                          c_vp, c_long, c_vp, c_long, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_int, c_vp, c_long,
                          c_int, c_int, c_vp],
    "kair_rowgemm_store": [c_vp, c_long, c_long, c_int, c_vp, c_int, c_vp, c_long, c_vp],
    "kair_rowgemm_gate": [c_vp, c_long, c_long, c_int, c_vp, c_int, c_vp, c_long, c_vp, c_long, c_vp],
    "kair_rowgemm_ln_blocks": [c_long, c_int],
    "kair_rowgemm_lnbwd": [c_vp, c_long, c_long, c_int, c_vp, c_vp, c_long, c_vp, c_vp, c_vp, c_int, c_vp, c_long,
                           c_int, c_int, c_int, c_int, ctypes.POINTER(CopyDesc), c_vp, c_vp],
    "kair_window_attn_fwd_x3": [c_vp, c_vp, c_vp, c_vp, c_vp, c_long, c_vp, c_long, c_int, c_int, c_float, c_int, c_int,
                                c_int, c_int, c_int, c_int, c_vp],
    "kair_window_attn_bwd_x3": [c_vp, c_vp, c_vp, c_vp, c_long, c_vp, c_vp, c_long, c_vp, c_vp, c_vp, c_vp, c_vp, c_int,
                                c_vp, c_long, c_int, c_int, c_float, c_int, c_int, c_int, c_int, c_int, c_vp],
    "kair_qkvblk_colsum_ws": [c_int],
    "kair_qkvblk_colsum": [c_vp, c_int, c_long, c_int, c_int, c_vp, c_vp, c_int, c_vp],
    "kair_table_transpose": [c_vp, c_vp, c_int, c_int, c_int, c_vp],
    "kair_scu_block_fwd": [c_vp, c_long, c_vp, c_long, c_vp, c_vp, c_vp, c_vp, c_float, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                           c_vp, c_vp, c_vp, c_float, c_int, c_int, c_int, c_int, c_int, c_vp],
    "kair_last_error": [],
    "kair_device_arch": [ctypes.c_char_p, c_int],
}
_RESTYPE = {"kair_gemm_nt_x3_lnbwd_parts": c_long, "kair_layernorm_bwd_blocks": c_long, "kair_rowgemm_ln_blocks": c_long, "kair_window_attn_bwd_groups": c_long, "kair_wgrad_grouped_ws": c_long, "kair_swin_mlp_bwd_ws": c_long, "kair_bn_ws": c_long, "kair_colsum_ws": c_long, "kair_last_error": ctypes.c_char_p, "kair_window_attn_bwd_ws": c_long, "kair_window_attn_bwd_ws_w": c_long, "kair_pack_table_bytes": c_long,
            "kair_pack_table_build": c_long, "kair_conv3x3_narrow_wgrad_ws": c_long,
            "kair_conv3x3_narrow_dgrad_ws": c_long, "kair_conv3x3_narrow_x3_ws": c_long,
            "kair_jpeg_workspace_bytes": c_long, "kair_ssim_workspace_bytes": c_long,
            "kair_grad_norm_ws": c_long, "kair_image_metrics_workspace_bytes": c_long,
            "kair_psnr_db_ref": ctypes.c_double,
            "kair_qkvblk_colsum_ws": c_long}

_lib = None


def lib():
    """Load libkair_hip.so once.  Raises RuntimeError (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"kair_amd: HIP kernel library not built ({LIB_PATH}); run `python -m kair_amd.build`")
        L = ctypes.CDLL(LIB_PATH)
        for name, args in _SIGS.items():
            if (name.startswith("kair_debug_") or os.environ.get("KAIR_LIB") == "base") and not hasattr(L, name):
                continue   # perf-investigation entry points, and an A/B baseline build's older symbol set
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = _RESTYPE.get(name, c_int)
        _lib = L
    return _lib


def exported_symbols():
    return list(_SIGS)


def check(rc, what=""):
    if rc != 0:
        msg = lib().kair_last_error().decode(errors="replace")
        raise RuntimeError(f"kair_hip {what} failed ({rc}): {msg}")


def ptr(t):
    if t is None:
        return None
    return t.data_ptr()


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def dtype_code(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float16:
        return F16
    raise TypeError(f"unsupported dtype {t.dtype}")


def require_device(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("kair_amd runs on the HIP device only (got a CPU tensor); there is no CPU fallback")


# ------------------------------------------------------------------------------------------
# descriptor builders
# ------------------------------------------------------------------------------------------
def rows(t, ld=None, win=None, rowscale=None, rows_per_scale=1, ones_col=-1, ones_in_data=False, w_split=False):
    """Row-major operand; win = (H, W, ws, shift) applies the Swin window->token row map.
    w_split: packed hi/lo bf16 weight rows (pack kind 9; gemm_nt B operand only)."""
    o = Operand()
    o._keep = (t, rowscale)  # keep the tensors alive until the launch has been issued
    o.ptr = ptr(t)
    o.dtype = dtype_code(t)
    o.mode = LD_ROWS
    o.ld = ld if ld is not None else t.shape[-1]
    if win:
        o.win_H, o.win_W, o.win_ws, o.win_shift = win
    o.rowscale = ptr(rowscale)
    o.rows_per_scale = rows_per_scale
    o.ones_col = ones_col
    o.ones_in_data = int(ones_in_data)
    o.w_split = int(w_split)
    return o


def asplit(op, lo=None, pair=False):
    """Mark a kair_gemm_nt A operand as a hi/lo activation pair: fp32 A forms lo in the kernel, a bf16 A
    (the hi plane) reads lo from `lo` (its producer's epilogue out_lo).  pair=True: the bf16 image's
    channels already are the [hi | lo] halves (weights packed tied over them; a_split 2)."""
    op.a_split = 2 if pair else 1
    if lo is not None:
        op.lo_ptr = ptr(lo)
        op._keep = (op._keep, lo)
    return op


def im2col(t, H, W, C, flip=False, ones_col=-1, ld=None, up=1, ones_in_data=False, dil=1):
    """3x3 / pad 1 im2col view of an NHWC map: H x W is the CONV grid, ld the pixel stride
    (default C), up=2 reads the source (H/2 x W/2) through a nearest x2 upsample.  ones_in_data: the
    map already holds 1.0 in channel ones_col % C of every pixel (read through the center tap,
    ones_col = 4 * C + c, by the tap-per-tile weight-gradient ring).  dil: the conv's dilation (padding =
    dilation, 1..4; kair_operand.im_dil): tap (dy, dx) reads pixel (y + dil dy, x + dil dx)."""
    o = Operand()
    o._keep = t
    o.ptr = ptr(t)
    o.dtype = dtype_code(t)
    o.mode = LD_IM2COL3
    o.ld = ld if ld is not None else C
    o.im_H, o.im_W, o.im_C, o.im_flip = H, W, C, int(flip)
    o.im_up = up
    o.im_dil = 0 if dil == 1 else dil   # 1: the field stays as every earlier caller left it
    o.ones_col = ones_col
    o.ones_in_data = int(ones_in_data)
    o.rows_per_scale = 1
    return o


def s2d(t, H, W, C, ld=None):
    """2x2 / stride-2 space-to-depth view of an NHWC map: H x W is the OUTPUT grid (the source is
    2H x 2W), column k = (i*2 + j) * C + c reads pixel (2y+i, 2x+j), channel c.  compute X3: an fp32 map,
    C % 8 == 0, K = 4 C (gemm_nt A / gemm_tn B)."""
    o = Operand()
    o._keep = t
    o.ptr = ptr(t)
    o.dtype = dtype_code(t)
    o.mode = LD_S2D
    o.ld = ld if ld is not None else C
    o.im_H, o.im_W, o.im_C = H, W, C
    o.ones_col = -1
    o.rows_per_scale = 1
    return o


def qkvblk(t, nh, hdp=32, tok=None, rowscale=None, rows_per_scale=1, ws=8):
    """Head-blocked q/k/v rows [3][nWin][nh][tok][hdp]; tok defaults to the ws * ws tokens of a window."""
    tok = ws * ws if tok is None else tok
    o = Operand()
    o._keep = (t, rowscale)
    o.ptr = ptr(t)
    o.dtype = dtype_code(t)
    o.mode = LD_QKVBLK
    o.qkv_nh, o.qkv_hdp, o.qkv_tok = nh, hdp, tok
    o.rowscale = ptr(rowscale)
    o.rows_per_scale = rows_per_scale
    o.ones_col = -1
    return o


def epilogue(out, mode=OUT_ROWS, ldo=None, win=None, bias=None, act=ACT_NONE, slope=0.0, pre=None, ldp=None,
             resid=None, ldr=None, rowscale=None, rows_per_scale=1, gate=None, ldg=None, gate_kind=0,
             ps=None, qkv=None, img=None, ones_col=-1, resid2=None, ldr2=None, pre_grad=False, acopy=None, out_lo=None):
    """pre_grad: `pre` receives act'(x) instead of x (GELU; read back with gate_kind=4).  acopy = (bf16
    tensor, ones_col): the 3x3 halo conv also writes its A image there (ones_col >= 0: that channel 1.0).
    out_lo: bf16 lo plane bf16(v - bf16(v)) beside a bf16 ROWS / PSHUF_SPM out (same layout)."""
    e = Epilogue()
    e.pre_kind = int(bool(pre_grad))
    e._keep = (out, bias, pre, resid, rowscale, gate, img, resid2, acopy, out_lo)
    e.out_lo = ptr(out_lo)
    if acopy is not None:
        e.a_copy, e.ld_acopy, e.acopy_ones_col_p1 = ptr(acopy[0]), acopy[0].shape[-1], acopy[1] + 1
    if resid2 is not None:
        e.resid2, e.ldr2 = ptr(resid2), (ldr2 if ldr2 is not None else resid2.shape[-1])
    e.out = ptr(out)
    e.out_dtype = dtype_code(out)
    e.out_mode = mode
    e.out_ones_col_p1 = ones_col + 1
    e.ldo = ldo if ldo is not None else out.shape[-1]
    if win:
        e.win_H, e.win_W, e.win_ws, e.win_shift = win
    e.bias = ptr(bias)
    e.act, e.slope = act, slope
    if pre is not None:
        e.out_pre, e.pre_dtype, e.ldp = ptr(pre), dtype_code(pre), (ldp if ldp is not None else pre.shape[-1])
    if resid is not None:
        e.resid, e.ldr = ptr(resid), (ldr if ldr is not None else resid.shape[-1])
    e.rowscale, e.rows_per_scale = ptr(rowscale), rows_per_scale
    if gate is not None:
        e.gate, e.gate_dtype, e.ldg, e.gate_kind = ptr(gate), dtype_code(gate), (ldg if ldg is not None else gate.shape[-1]), gate_kind
    if ps:
        e.ps_r, e.ps_H, e.ps_W = ps
    if qkv:
        e.qkv_nh, e.qkv_hdp, e.qkv_tok = qkv
    if img:
        mean, rng, C, H, W = img
        e.img_mean, e.img_range, e.img_C, e.img_H, e.img_W = ptr(mean), rng, C, H, W
    return e


def wmap(kind, N, K, n_groups=(1, None, None), k_groups=(1, None, None), n_perm=0):
    """n_groups = (G, real, padded) for the out dim; k_groups likewise for the in dim; n_perm = r*r
    stores the out dim sub-pixel-major (PixelShuffle SPM layouts).  Kinds: kair_wmap (kair_hip.h); the x3
    fp16-pair forms are 9 / 17 / 18 / 19 (3x3 forward, linear, 3x3 dgrad, transposed linear), 20 / 21 (the
    2x2 forms 7 / 8) and 22 / 23 (3x3 forward / dgrad in 16x16x32 fragment order: conv3x3_wr_x3)."""
    m = WMap()
    m.kind, m.N, m.K = kind, N, K
    m.n_perm = n_perm
    nG, nr, npd = n_groups
    kG, kr, kpd = k_groups
    m.nG, m.nGr, m.nGp = nG, nr or N // nG, npd or nr or N // nG
    m.kG, m.kGr, m.kGp = kG, kr or (K // kG if K else 1), kpd or kr or (K // kG if K else 1)
    return m


# ------------------------------------------------------------------------------------------
# thin call wrappers (raise on error)
# ------------------------------------------------------------------------------------------
def gemm_nt(A, B, E, M, N, K, compute):
    check(lib().kair_gemm_nt(ctypes.byref(A), ctypes.byref(B), ctypes.byref(E), M, N, K, compute, stream_ptr()), "gemm_nt")


def conv_halo_geometry(H, W, C, M, N):
    """True when a bf16 3x3 conv of this geometry runs on the halo path (can write epilogue acopy)."""
    return bool(lib().kair_conv3x3_halo_geometry(H, W, C, M, N))


def wgrad_splits(M, N, K):
    return lib().kair_wgrad_splits(M, N, K)


def wgrad_tiles(N, K):
    """(N, K) tiles of one kair_gemm_tn split (the launch has tiles x splits workgroups): the 192 x 192
    ring tile where it applies, a 192-wide N tile for N in (128, 192], else 128 x 128 (gemm.hip)."""
    if N <= 576 and K <= 576 and N % 8 == 0 and K % 8 == 0 and N > 64 and K > 64:
        return -(-N // 192) * -(-K // 192)
    if N <= 576 and N % 8 == 0 and N > 64 and K == 9 * 192:   # conv weight gradient, one tap per tile
        return -(-N // 192) * 9
    if N <= 64 and K <= 64:
        return 1
    if 128 < N <= 192 and K > 128:
        return -(-K // 128)
    return -(-N // 128) * -(-K // 128)


def gemm_tn(A, B, ws, splits, M, N, K, compute):
    check(lib().kair_gemm_tn(ctypes.byref(A), ctypes.byref(B), ptr(ws), splits, M, N, K, compute, stream_ptr()), "gemm_tn")


def wgrad_grouped_ws(shapes, M, x3=False):
    """Workspace floats of a kair_wgrad_grouped launch over linears of packed (N, K) shapes (x3: fp16-pair jobs,
    the fp32x3 TN ring's 192 x 192 tiles)."""
    arr = (WgradJob * len(shapes))()
    for i, (N, K) in enumerate(shapes):
        arr[i].N, arr[i].K = N, K
        arr[i].A.dtype = F16 if x3 else BF16
    return lib().kair_wgrad_grouped_ws(arr, len(shapes), M)


class WgradGroup:
    """The weight gradients of several linear layers (kair_wgrad_grouped): one TN launch + one
    finalize launch.  jobs: (A operand, B operand, N, K, wmap, grad, bias_grad or None, ones_col)."""

    WG_MAX = 24

    def __init__(self, jobs, M):
        if not 0 < len(jobs) <= self.WG_MAX:
            raise ValueError(f"kair_wgrad_grouped: 1..{self.WG_MAX} jobs (got {len(jobs)})")
        arr = (WgradJob * len(jobs))()
        for i, (A, B, N, K, m, grad, bias, oc) in enumerate(jobs):
            arr[i].A, arr[i].B, arr[i].N, arr[i].K, arr[i].map = A, B, N, K, m
            arr[i].grad, arr[i].bias_grad, arr[i].ones_col = ptr(grad), ptr(bias), oc
        self._keep = jobs
        self.arr, self.n, self.M = arr, len(jobs), M
        self.ws_floats = lib().kair_wgrad_grouped_ws(arr, self.n, M)

    def run(self, ws, max_ctas=0):
        """max_ctas > 0: at most that many workgroups (kair_wgrad_grouped_ex: fewer row splits); < 0:
        -max_ctas times the default splits (the workspace scales with it)."""
        if ws.numel() < self.ws_floats * max(1, -max_ctas):
            raise ValueError("kair_wgrad_grouped: workspace too small")
        check(lib().kair_wgrad_grouped_ex(self.arr, self.n, self.M, ptr(ws), int(max_ctas), stream_ptr()),
              "wgrad_grouped")


def pack_weight(src, dst, m):
    check(lib().kair_pack_weight(ptr(src), ptr(dst), dtype_code(dst), ctypes.byref(m), stream_ptr()), "pack_weight")


class PackTable:
    """Every (src, dst, map) re-pack of a network, launched as ONE kernel (kair_pack_weights)."""

    def __init__(self, jobs):
        n = len(jobs)
        arr = (PackJob * n)()
        for i, (src, dst, m) in enumerate(jobs):
            arr[i].src, arr[i].dst, arr[i].dst_dtype, arr[i].map = ptr(src), ptr(dst), dtype_code(dst), m
        self._keep = [(s, d) for s, d, _ in jobs]
        self.n = n
        self.table = torch.empty(lib().kair_pack_table_bytes(n), dtype=torch.uint8, device=jobs[0][1].device)
        nb = lib().kair_pack_table_build(arr, n, ptr(self.table))
        if nb <= 0:
            check(int(nb) or -1, "pack_table_build")
        self.nblocks = nb

    def run(self):
        check(lib().kair_pack_weights(ptr(self.table), self.n, self.nblocks, stream_ptr()), "pack_weights")


def wgrad_finalize(partial, splits, m, grad, bias_grad=None, ones_col=-1, accumulate=False):
    check(lib().kair_wgrad_finalize(ptr(partial), splits, ctypes.byref(m), ptr(grad), ptr(bias_grad), ones_col,
                                    int(accumulate), stream_ptr()), "wgrad_finalize")


_COLSUM_WS = {}


def colsum_ws(Np):
    """Workspace floats of a kair_colsum launch over Np columns: every partial sum it writes (cached per Np)."""
    n = _COLSUM_WS.get(Np)
    if n is None:
        n = _COLSUM_WS[Np] = lib().kair_colsum_ws(Np)
    return n


def colsum(G, M, Np, m, bias_grad, ws, accumulate=False):
    if ws.numel() < colsum_ws(Np):
        raise ValueError(f"kair_colsum: workspace too small for Np = {Np} ({ws.numel()} < {colsum_ws(Np)} floats)")
    check(lib().kair_colsum(ctypes.byref(G), M, Np, ctypes.byref(m), ptr(bias_grad), ptr(ws), int(accumulate),
                            stream_ptr()), "colsum")


def layernorm_fwd(x, ldx, y, ldy, gamma, beta, mean, rstd, M, C, eps=1e-5, win=(0, 0, 0, 0), one_col=-1):
    check(lib().kair_layernorm_fwd(ptr(x), ldx, ptr(y), dtype_code(y), ldy, ptr(gamma), ptr(beta), ptr(mean), ptr(rstd),
                                   M, C, eps, *win, one_col, stream_ptr()), "layernorm_fwd")


def layernorm_fwd_x3(x, ldx, y, ldy, gamma, beta, mean, rstd, M, C, eps=1e-5, win=(0, 0, 0, 0), one_col=-1, x3_exp=0):
    """LayerNorm forward into an fp16 pair y [2, M, ldy] (hi, lo planes) of y 2^x3_exp (the fp32x3 GEMM operand)."""
    check(lib().kair_layernorm_fwd_x3(ptr(x), ldx, ptr(y[0]), ptr(y[1]), ldy, ptr(gamma), ptr(beta), ptr(mean), ptr(rstd),
                                      M, C, eps, *win, one_col, int(x3_exp), stream_ptr()), "layernorm_fwd_x3")


def layernorm_bwd(x, ldx, dy, ldy, gamma, mean, rstd, dx, ld_dx, dx_acc, dgamma, dbeta, dparam_acc, ws, M, C,
                  win=(0, 0, 0, 0), copy=None):
    check(lib().kair_layernorm_bwd(ptr(x), ldx, ptr(dy), dtype_code(dy), ldy, ptr(gamma), ptr(mean), ptr(rstd), ptr(dx),
                                   ld_dx, int(dx_acc), ptr(dgamma), ptr(dbeta), int(dparam_acc), ptr(ws), M, C, *win,
                                   ctypes.byref(copy) if copy is not None else None, stream_ptr()), "layernorm_bwd")


def gemm_nt_lnbwd(A, B, M, N, K, x, ldx, gamma, mean, rstd, C, D, ldd, part, win=(0, 0, 0, 0), copy=None):
    """fp32x3: dxn = A B^T fused with the LayerNorm backward (kair_gemm_nt_x3_lnbwd): D[t] += LN'(dxn), the optional
    fp16-pair copy of D, dgamma / dbeta partial rows in part (gemm_nt_lnbwd_parts(M, N) rows of 2 C)."""
    check(lib().kair_gemm_nt_x3_lnbwd(ctypes.byref(A), ctypes.byref(B), M, N, K, *win, ptr(x), ldx, ptr(gamma), ptr(mean),
                                      ptr(rstd), C, ptr(D), ldd, ptr(part),
                                      ctypes.byref(copy) if copy is not None else None, stream_ptr()), "gemm_nt_x3_lnbwd")


def gemm_nt_lnbwd_parts(M, N):
    return lib().kair_gemm_nt_x3_lnbwd_parts(M, N)


def row_copy(src, ld_src, M, C, copy):
    check(lib().kair_row_copy(ptr(src), ld_src, M, C, ctypes.byref(copy), stream_ptr()), "row_copy")


def window_attn_fwd(qkv, table, O, ldo, lse, nWin, nh, hd, scale, H, W, shift, ones_col=-1, mask=None, head_pad=32, ws=8):
    """head_pad: 32, or 16 (bf16, head_dim <= 16): the per-head width of the qkv / O layouts.
    ws: the window size, 8 or 7 (49 tokens per window in every layout)."""
    mnw = mask.shape[0] if mask is not None else 0
    check(lib().kair_window_attn_fwd_w(ptr(qkv), dtype_code(qkv), ptr(table), ptr(O), ldo, ptr(lse), nWin, nh, hd, scale,
                                       H, W, shift, ones_col, ptr(mask), mnw, head_pad, ws, stream_ptr()), "window_attn_fwd")


GROUP_MAX = 32   # jobs per kair_ln_param_reduce_grouped / kair_attn_dtable_grouped launch (LNP_MAX, DTAB_MAX)


def layernorm_bwd_blocks(M):
    return lib().kair_layernorm_bwd_blocks(M)


def ln_param_reduce_grouped(jobs):
    """jobs: (partials left by layernorm_bwd(dgamma=None, dbeta=None), M, C, dgamma, dbeta, accumulate[, nb]);
    nb (the partial-row count) defaults to layernorm_bwd's for M (rowgemm_lnbwd: rowgemm_ln_blocks)."""
    arr = (LnParamJob * len(jobs))()
    for i, job in enumerate(jobs):
        part, M, C, dg, db, acc = job[:6]
        nb = job[6] if len(job) > 6 else layernorm_bwd_blocks(M)
        arr[i].part, arr[i].nb, arr[i].C = ptr(part), nb, C
        arr[i].dgamma, arr[i].dbeta, arr[i].accumulate = ptr(dg), ptr(db), int(acc)
    check(lib().kair_ln_param_reduce_grouped(arr, len(jobs), stream_ptr()), "ln_param_reduce_grouped")


def attn_dtable_grouped(jobs):
    """jobs: (ws left by window_attn_bwd(dtable=None), nWin, nh, dtype code, dtable, accumulate[, window size])."""
    arr = (DtabJob * len(jobs))()
    for i, job in enumerate(jobs):
        ws, nWin, nh, dt, dtable, acc = job[:6]
        arr[i].ws, arr[i].nWin, arr[i].nh, arr[i].dtype = ptr(ws), nWin, nh, dt
        arr[i].dtable, arr[i].accumulate = ptr(dtable), int(acc)
        arr[i].win_ws = job[6] if len(job) > 6 else 0
    check(lib().kair_attn_dtable_grouped(arr, len(jobs), stream_ptr()), "attn_dtable_grouped")


def window_attn_bwd_ws(nWin, nh, ws=8):
    if ws not in (7, 8):
        raise ValueError(f"window_attn_bwd_ws: window size {ws} (7 or 8)")
    return lib().kair_window_attn_bwd_ws_w(nWin, nh, ws)


def window_attn_bwd(qkv, O, ldo, dO, lddo, table, lse, dqkv, dtable, dtable_acc, ws, nWin, nh, hd, scale, H, W, shift,
                    mask=None, dqkv_rows=False, head_pad=32, win_ws=8):
    """dqkv_rows: dqkv as token rows [nWin*64, 3*nh*head_pad] (bf16) instead of head-blocked.  win_ws: the window
    size, 8 or 7 (`ws` is the partials workspace)."""
    mnw = mask.shape[0] if mask is not None else 0
    check(lib().kair_window_attn_bwd_w(ptr(qkv), ptr(O), ldo, ptr(dO), lddo, dtype_code(qkv), ptr(table), ptr(lse),
                                       ptr(dqkv), int(dqkv_rows), ptr(dtable), int(dtable_acc), ptr(ws), nWin, nh, hd,
                                       scale, H, W, shift, ptr(mask), mnw, head_pad, win_ws, stream_ptr()), "window_attn_bwd")


def _planes(t):
    """(hi, lo) pointers of an x3 tensor: an fp16 pair [2, ...] or an fp32 tensor in natural units (lo NULL)."""
    return (ptr(t), None) if t.dtype == torch.float32 else (ptr(t[0]), ptr(t[1]))


def window_attn_fwd_x3(qkv, table, O, ldo, lse, nWin, nh, hd, scale, H, W, shift, ones_col=-1, e_in=0, e_out=0, ws=8):
    """Split-fp16 window attention forward: qkv is [2, ...] fp16 (hi plane, lo plane) of x 2^e_in; O the same
    with e_out, or an fp32 tensor (natural units)."""
    o, ol = _planes(O)
    check(lib().kair_window_attn_fwd_x3_w(ptr(qkv[0]), ptr(qkv[1]), ptr(table), o, ol, ldo, ptr(lse), nWin,
                                          nh, hd, scale, H, W, shift, ones_col, e_in, e_out, ws, stream_ptr()),
          "window_attn_fwd_x3")


def window_attn_bwd_x3(qkv, O, ldo, dO, lddo, table, lse, dqkv, dtable, dtable_acc, ws, nWin, nh, hd, scale, H, W, shift,
                       e_act=0, e_grad=0, win_ws=8):
    """Split-fp16 window attention backward: qkv, dO are [2, ...] fp16 planes; O and dqkv (token rows [M][3 nh 32])
    fp16 pairs or fp32 (natural units); q/k/v and O pairs carry e_act, dO and a dqkv pair e_grad."""
    o, ol = _planes(O)
    dq, dql = _planes(dqkv)
    check(lib().kair_window_attn_bwd_x3_w(ptr(qkv[0]), ptr(qkv[1]), o, ol, ldo, ptr(dO[0]), ptr(dO[1]), lddo,
                                          ptr(table), ptr(lse), dq, dql, ptr(dtable), int(dtable_acc),
                                          ptr(ws), nWin, nh, hd, scale, H, W, shift, e_act, e_grad, win_ws, stream_ptr()),
          "window_attn_bwd_x3")


def with_lo(op, lo):
    """Attach the lo plane of a 16-bit operand pair (split-fp16 GEMMs of kair_gemm_nt / kair_gemm_tn compute X3;
    the bf16 engine's a_split)."""
    op.lo_ptr = ptr(lo)
    op._keep = (op._keep, lo)
    return op


def conv3x3_narrow_fwd(x, ldx, lo_off, w, bias, NR, mean, img_range, resid, out, B, H, W):
    """conv_last forward: 64-channel bf16 rows (hi, + lo at lo_off) -> NCHW image (csrc/tail.hip)."""
    check(lib().kair_conv3x3_narrow_fwd(ptr(x), ldx, lo_off, ptr(w), ptr(bias), NR, ptr(mean), img_range, ptr(resid),
                                        ptr(out), B, H, W, stream_ptr()), "conv3x3_narrow_fwd")


def conv3x3_wr_tile(split, B, H, W, C, N):
    """Tile (pixels) of kair_conv3x3_wr for this shape, 0 when unsupported."""
    return lib().kair_conv3x3_wr_tile(int(bool(split)), B, H, W, C, N)


def conv3x3_wr(x, ldx, flip, w, bias, resid, out, B, H, W, C, N, ldr=None, ldo=None, acopy=None, ldac=None, acones=-1,
               n_blocks=None, split=None, out_lo=None, ps_r=0, act=ACT_NONE, slope=0.0, gate=None, ldg=None):
    """3x3 conv with register-streamed weights (csrc/conv_wr.hip, kair_conv3x3_wr_ex).  split (default: x
    fp32): two halos -- split activations of an fp32 image, or a bf16 [hi | lo] pair image of C channels
    per half -- with w = pack kind 15; else one bf16 product with w = pack kind 16 (flip = 1: input
    gradient).  ps_r > 0: PixelShuffle sub-pixel-major store (+ out_lo: the lo plane of a bf16 pair); ps_r < 0:
    PixelUnshuffle(-ps_r) store; gate: LeakyReLU'(gate) (slope) on the rows."""
    if split is None:
        split = x.dtype == torch.float32
    if n_blocks is None:
        n_blocks = 16 if N > 192 else 12 if N > 64 else 4
    check(lib().kair_conv3x3_wr_ex(ptr(x), dtype_code(x), ldx, int(bool(split)), int(flip), ptr(w), n_blocks, ptr(bias),
                                   ptr(resid), ldr if ldr is not None else (resid.shape[-1] if resid is not None else 0),
                                   ptr(out), dtype_code(out), ldo if ldo is not None else out.shape[-1], ptr(out_lo), ps_r,
                                   act, slope, ptr(gate), ldg if ldg is not None else (gate.shape[-1] if gate is not None else 0),
                                   ptr(acopy), ldac if ldac is not None else (acopy.shape[-1] if acopy is not None else 0),
                                   acones, B, H, W, C, N, stream_ptr()), "conv3x3_wr")


def conv3x3_dil_ok(dil, C, N):
    """Whether kair_conv3x3_dil takes this conv (dilation 2..4, C = N = 64)."""
    return bool(lib().kair_conv3x3_dil_ok(dil, C, N))


def conv3x3_dil(x, ldx, dil, flip, w, w_kind, bias, out, B, H, W, C, N, ldo=None, act=ACT_NONE, slope=0.0):
    """Dilated 3x3 conv over bf16 NHWC rows (csrc/conv_dil.hip): w = pack kind 15 (forward) or 16 (flip = 1: input
    gradient); out fp32 or bf16 rows of stride ldo."""
    check(lib().kair_conv3x3_dil(ptr(x), ldx, dil, int(flip), ptr(w), w_kind, ptr(bias), act, slope, ptr(out),
                                 dtype_code(out), ldo if ldo is not None else out.shape[-1], B, H, W, C, N, stream_ptr()),
          "conv3x3_dil")


def conv3x3_wr_x3_tile(B, H, W, C, N):
    """Tile (pixels) of kair_conv3x3_wr_x3 for this shape, 0 when unsupported."""
    return lib().kair_conv3x3_wr_x3_tile(B, H, W, C, N)


def conv3x3_wr_x3(x, ldx, x3_exp, flip, w, bias, resid, out, B, H, W, C, N, ldr=None, ldo=None):
    """kair_conv3x3_wr_x3: the fp16-pair 3x3 conv with register-streamed weights on fp32 rows x (scaled by
    2^x3_exp in the kernel); w = fp16 pack kind 22, or 23 with flip = 1 for an input gradient."""
    if x.dtype != torch.float32 or out.dtype != torch.float32 or w.dtype != torch.float16:
        raise TypeError("conv3x3_wr_x3: fp32 rows in and out, fp16 packed weights")
    check(lib().kair_conv3x3_wr_x3(ptr(x), ldx, int(x3_exp), int(flip), ptr(w), 12, ptr(bias), ptr(resid),
                                   ldr if ldr is not None else (resid.shape[-1] if resid is not None else 0), ptr(out),
                                   ldo if ldo is not None else out.shape[-1], B, H, W, C, N, stream_ptr()), "conv3x3_wr_x3")


def conv3x3_narrow_dgrad_ws():
    return lib().kair_conv3x3_narrow_dgrad_ws()


def conv3x3_narrow_dgrad(dE, lde, w, NR, ws, out, ldo, ps_r, B, H, W):
    check(lib().kair_conv3x3_narrow_dgrad(ptr(dE), lde, ptr(w), NR, ptr(ws), ptr(out), dtype_code(out), ldo, ps_r, B, H, W,
                                          stream_ptr()), "conv3x3_narrow_dgrad")


def conv3x3_narrow_wgrad_ws(NR):
    return lib().kair_conv3x3_narrow_wgrad_ws(NR)


def conv3x3_narrow_wgrad(dE, lde, x, ldx, NR, ws, grad_w, grad_b, B, H, W, accumulate=False):
    check(lib().kair_conv3x3_narrow_wgrad(ptr(dE), lde, ptr(x), ldx, NR, ptr(ws), ptr(grad_w), ptr(grad_b),
                                          int(accumulate), B, H, W, stream_ptr()), "conv3x3_narrow_wgrad")


def conv3x3_narrow_x3_ws():
    return lib().kair_conv3x3_narrow_x3_ws()


def conv3x3_narrow_fwd_x3(x, ldx, ex, w, bias, NR, ws, mean, img_range, resid, out, B, H, W):
    """conv_last forward at the fp32 engine's arithmetic: 64-channel fp32 rows -> NCHW image (csrc/tail.hip)."""
    check(lib().kair_conv3x3_narrow_fwd_x3(ptr(x), ldx, ex, ptr(w), ptr(bias), NR, ptr(ws), ptr(mean), img_range, ptr(resid),
                                           ptr(out), B, H, W, stream_ptr()), "conv3x3_narrow_fwd_x3")


def conv3x3_narrow_dgrad_x3(dE, lde, eg, w, NR, ws, out, ldo, ps_r, B, H, W):
    check(lib().kair_conv3x3_narrow_dgrad_x3(ptr(dE), lde, eg, ptr(w), NR, ptr(ws), ptr(out), ldo, ps_r, B, H, W,
                                             stream_ptr()), "conv3x3_narrow_dgrad_x3")


def conv3x3_narrow_wgrad_x3(dE, lde, eg, x, ldx, ex, NR, ws, grad_w, grad_b, B, H, W, accumulate=False):
    check(lib().kair_conv3x3_narrow_wgrad_x3(ptr(dE), lde, eg, ptr(x), ldx, ex, NR, ptr(ws), ptr(grad_w), ptr(grad_b),
                                             int(accumulate), B, H, W, stream_ptr()), "conv3x3_narrow_wgrad_x3")


def image_to_nhwc_hilo(img, out, ldc, mean, img_range, B, C, H, W):
    """bf16 hi/lo pair of the normalised image: hi in channels [0, C), lo in [ldc/2, ldc/2 + C)."""
    check(lib().kair_image_to_nhwc_hilo(ptr(img), ptr(out), ldc, ptr(mean), img_range, B, C, H, W, stream_ptr()),
          "image_to_nhwc_hilo")


def image_to_nhwc(img, out, ldc, mean, img_range, B, C, H, W):
    check(lib().kair_image_to_nhwc(ptr(img), ptr(out), dtype_code(out), ldc, ptr(mean), img_range, B, C, H, W,
                                   stream_ptr()), "image_to_nhwc")


def ffd_pack(img, sigma, out, ldc, B, C, H, W):
    """FFDNet's PixelUnshuffle(2) head (kair_ffd_pack): img [B, C, H, W] fp32 -> out rows [B * ceil(H/2) * ceil(W/2), ldc]
    (fp32 / bf16).  sigma [B] fp32: replicate-padded input pack with the level in channel 4C; sigma None: the
    zero-padded pack of an output gradient."""
    require_device(img, out, sigma)
    if img.dtype != torch.float32 or not img.is_contiguous() or tuple(img.shape) != (B, C, H, W):
        raise ValueError(f"ffd_pack: img must be a contiguous fp32 {(B, C, H, W)}")
    if sigma is not None and (sigma.dtype != torch.float32 or not sigma.is_contiguous() or sigma.numel() != B):
        raise ValueError(f"ffd_pack: sigma must be {B} contiguous fp32 levels")
    if not out.is_contiguous() or out.numel() < B * ((H + 1) // 2) * ((W + 1) // 2) * ldc:
        raise ValueError("ffd_pack: out is smaller than the packed rows")
    check(lib().kair_ffd_pack(ptr(img), ptr(sigma), ptr(out), dtype_code(out), ldc, B, C, H, W, stream_ptr()), "ffd_pack")


def l1_loss(E, H, loss_out, dE, ldc, weight, B, C, Hh, Ww, ws, ps_r=1, charb_eps=None):
    """L1 (mean) loss + its gradient; charb_eps set: the Charbonnier loss sqrt(d^2 + eps) instead."""
    if charb_eps is not None:
        check(lib().kair_charbonnier_loss(ptr(E), ptr(H), ptr(loss_out), ptr(dE), dtype_code(dE), ldc, ps_r, weight,
                                          float(charb_eps), B, C, Hh, Ww, ptr(ws), stream_ptr()), "charbonnier_loss")
        return
    check(lib().kair_l1_loss(ptr(E), ptr(H), ptr(loss_out), ptr(dE), dtype_code(dE), ldc, ps_r, weight, B, C, Hh, Ww,
                             ptr(ws), stream_ptr()), "l1_loss")


def ssim_workspace_bytes(B, C, Hh, Ww):
    """kair_ssim_workspace_bytes: the workspace of one ssim_loss call on [B, C, Hh, Ww] images."""
    return lib().kair_ssim_workspace_bytes(B, C, Hh, Ww)


def ssim_workspace(B, C, Hh, Ww, device):
    return torch.empty(ssim_workspace_bytes(B, C, Hh, Ww), dtype=torch.uint8, device=device)


def ssim_loss(E, H, loss_out, dE, ldc, weight, B, C, Hh, Ww, ws, ps_r=1):
    """weight * mean SSIM(E, H) (the SSIM itself: maximising it takes a negative weight) + its gradient, in
    l1_loss's rows layout; ldc None: dE is the fp32 NCHW image gradient.  ws: ssim_workspace(B, C, Hh, Ww)."""
    if ws.numel() * ws.element_size() < ssim_workspace_bytes(B, C, Hh, Ww):
        raise ValueError(f"kair_ssim_loss: workspace too small ({ws.numel() * ws.element_size()} < "
                         f"{ssim_workspace_bytes(B, C, Hh, Ww)} bytes)")
    if ldc is None:
        if dE.dtype != torch.float32:
            raise TypeError("kair_ssim_loss_nchw: the image gradient is fp32")
        check(lib().kair_ssim_loss_nchw(ptr(E), ptr(H), ptr(loss_out), ptr(dE), weight, B, C, Hh, Ww, ptr(ws),
                                        stream_ptr()), "ssim_loss_nchw")
        return
    check(lib().kair_ssim_loss(ptr(E), ptr(H), ptr(loss_out), ptr(dE), dtype_code(dE), ldc, ps_r, weight, B, C, Hh, Ww,
                               ptr(ws), stream_ptr()), "ssim_loss")


METRIC_Y, METRIC_SSIM = 1, 2   # KAIR_METRIC_Y, KAIR_METRIC_SSIM


def image_metrics_workspace(B, C, Hh, Ww, border, flags, device):
    """The workspace of one image_metrics call (kair_image_metrics_workspace_bytes: one 16-byte slot per tile)."""
    nbytes = lib().kair_image_metrics_workspace_bytes(B, C, Hh, Ww, border, flags)
    if nbytes <= 0:
        raise ValueError(f"kair_image_metrics: no valid call on [{B}, {C}, {Hh}, {Ww}] images with border {border}, "
                         f"flags {flags}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def image_metrics(E, H, out, B, C, Hh, Ww, border, flags, ws):
    """kair_image_metrics: per image the exact uint8 SSE (out[b][0]) and, with METRIC_SSIM, the uint8 SSIM (out[b][1])
    of fp32 NCHW images; METRIC_Y: on the Y channel (C = 3).  out: float64 [B, 2]; ws: image_metrics_workspace(...)."""
    require_device(E, H, out, ws)
    if out.dtype != torch.float64 or out.numel() < 2 * B:
        raise TypeError("kair_image_metrics: out is a float64 [B, 2] tensor")
    need = lib().kair_image_metrics_workspace_bytes(B, C, Hh, Ww, border, flags)
    if ws.numel() * ws.element_size() < need:
        raise ValueError(f"kair_image_metrics: workspace too small ({ws.numel() * ws.element_size()} < {need} bytes)")
    check(lib().kair_image_metrics(ptr(E), ptr(H), ptr(out), B, C, Hh, Ww, border, flags, ptr(ws), stream_ptr()),
          "image_metrics")


def psnr_db(sse, db, count):
    """kair_psnr_db: db[i] = calculate_psnr's dB of the exact SSE sse[i] over `count` compared values (inf at 0), with
    the host C library's bits.  sse, db: float64 device tensors of one dimension (any stride; db may be sse)."""
    require_device(sse, db)
    if sse.dtype != torch.float64 or db.dtype != torch.float64 or sse.dim() != 1 or db.shape != sse.shape:
        raise TypeError("kair_psnr_db: sse and db are float64 vectors of one length")
    check(lib().kair_psnr_db(ptr(sse), max(1, sse.stride(0)), ptr(db), max(1, db.stride(0)), sse.numel(), float(count),
                             stream_ptr()), "psnr_db")


def psnr_db_ref(sse, count):
    """kair_psnr_db_ref: the same arithmetic evaluated on the host for one value."""
    return lib().kair_psnr_db_ref(float(sse), float(count))


def axpy(y, x, a, n=None):
    check(lib().kair_axpy(ptr(y), ptr(x), a, n if n is not None else y.numel(), stream_ptr()), "axpy")


def adam_ema(p, g, m, v, ema, n, lr_t, beta1, beta2, eps, wd, decay, skip=None):
    """skip: an int32 device flag (kair_range_check): nonzero drops the step (kair_adam_ema_ex)."""
    if skip is not None:
        check(lib().kair_adam_ema_ex(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), n, ptr(lr_t), beta1, beta2, eps, wd, decay,
                                     ptr(skip), stream_ptr()), "adam_ema_ex")
        return
    check(lib().kair_adam_ema(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), n, ptr(lr_t), beta1, beta2, eps, wd, decay,
                              stream_ptr()), "adam_ema")


def ktime_begin(n=4096):
    """Open a kernel timing window of n slots (kair_ktime_begin): every later libkair launch into a non-capturing
    stream is timed by its dispatch packet's start / end, as rocprofv3 --kernel-trace times it."""
    check(lib().kair_ktime_begin(n), "ktime_begin")


def ktime_count():
    return lib().kair_ktime_count()


def ktime_end():
    return lib().kair_ktime_end()


def gate_hold(timeout_ms=5000):
    """Hold the current stream behind one waiting wave until gate_release() (or timeout_ms): an eager pass queued
    behind it then runs back to back (kair_gate_hold)."""
    check(lib().kair_gate_hold(timeout_ms, stream_ptr()), "gate_hold")


def gate_release():
    check(lib().kair_gate_release(), "gate_release")


def gate_status():
    """0 pending, 1 released by the host, 2 the wave's time limit passed first."""
    return lib().kair_gate_status()


def ktime_read(i):
    """(duration ms, kernel symbol) of slot i of the last window; waits for that launch."""
    ms, name = ctypes.c_float(), ctypes.c_char_p()
    check(lib().kair_ktime_read(i, ctypes.byref(ms), ctypes.byref(name)), "ktime_read")
    return ms.value, (name.value or b"").decode(errors="replace")


def l2_loss(E, H, loss_out, dE, ldc, weight, B, C, Hh, Ww, ws, ps_r=1, reduction="mean"):
    """kair_l2_loss: weight * mean (reduction 'mean', nn.MSELoss()) or sum ('sum') of (E - H)^2 into loss_out, its
    gradient into the dE rows (l1_loss's layouts).  ws: 1024 floats."""
    if reduction not in ("mean", "sum"):
        raise ValueError(f"l2_loss: reduction {reduction!r} ('mean' or 'sum')")
    check(lib().kair_l2_loss(ptr(E), ptr(H), ptr(loss_out), ptr(dE), dtype_code(dE), ldc, ps_r, weight,
                             int(reduction == "sum"), B, C, Hh, Ww, ptr(ws), stream_ptr()), "l2_loss")


_GRAD_NORM_GEOM = None


def grad_norm_geometry():
    """(grid, block, workspace floats) of kair_grad_norm's first launch (kair_grad_norm_ws): fixed, whatever n is."""
    global _GRAD_NORM_GEOM
    if _GRAD_NORM_GEOM is None:
        g, b = c_int(0), c_int(0)
        n = lib().kair_grad_norm_ws(ctypes.byref(g), ctypes.byref(b))
        _GRAD_NORM_GEOM = (g.value, b.value, n)
    return _GRAD_NORM_GEOM


def grad_norm(g, ws, norm_out):
    """norm_out[0] = the 2-norm of the flat fp32 buffer g (kair_grad_norm); ws: grad_norm_geometry()[2] floats."""
    if g.dtype != torch.float32 or not g.is_contiguous():
        raise ValueError("grad_norm: g must be a contiguous fp32 tensor")
    if ws.numel() < grad_norm_geometry()[2]:
        raise ValueError(f"grad_norm: workspace too small ({ws.numel()} < {grad_norm_geometry()[2]} floats)")
    check(lib().kair_grad_norm(ptr(g), g.numel(), ptr(ws), ptr(norm_out), stream_ptr()), "grad_norm")


def adam_ema_clip(p, g, m, v, ema, n, lr_t, beta1, beta2, eps, wd, decay, gnorm, max_norm, skip=None):
    """adam_ema on g * min(1, max_norm / (gnorm[0] + 1e-6)) (kair_adam_ema_clip); a step that clips also leaves the
    clipped gradient in g.  gnorm: grad_norm's device result; skip as in adam_ema."""
    check(lib().kair_adam_ema_clip(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), n, ptr(lr_t), beta1, beta2, eps, wd, decay,
                                   ptr(skip), ptr(gnorm), float(max_norm), stream_ptr()), "adam_ema_clip")


def range_check(g, p, loss, p_limit, flag):
    """fp32x3 range guard: flag[0] = 1 (non-finite gradient) | 2 (non-finite loss) | 4 (|p| >= p_limit)."""
    check(lib().kair_range_check(ptr(g), ptr(p), g.numel(), ptr(loss), float(p_limit), ptr(flag), stream_ptr()),
          "range_check")


def axpby(y, x, a, b, n=None):
    """y = a * x + b * y (fp32)."""
    check(lib().kair_axpby(ptr(y), ptr(x), a, b, n if n is not None else y.numel(), stream_ptr()), "axpby")


def act_grad_cast(G, ldg, X, ldx, out, ldo, M, C, kind, slope=0.0, scale=1.0):
    """out = scale * G * act'(X) (act' read from the post-activation X; kind 0 none, 1 relu, 2 leaky)."""
    check(lib().kair_act_grad_cast(ptr(G), ldg, ptr(X), dtype_code(X) if X is not None else F32, ldx, ptr(out),
                                   dtype_code(out), ldo, M, C, kind, slope, scale, stream_ptr()), "act_grad_cast")


def sumpool2x(src, lds, dst, ldd, B, H, W, C, accumulate=False):
    """dst (+)= 2x2 sum-pool of src (the adjoint of nearest x2 upsampling)."""
    check(lib().kair_sumpool2x(ptr(src), lds, ptr(dst), ldd, B, H, W, C, int(accumulate), stream_ptr()), "sumpool2x")


def act_grad_punshuf(G, X, out, out_f32, B, H, W, C, r, kind, slope=0.0):
    """act_grad_cast through the inverse of a sub-pixel-major PixelShuffle(r): G fp32 / X dense rows [B H r W r, C] of
    the shuffled image -> out (and out_f32, or None) pre-shuffle rows [B H W, r r C]."""
    n = B * H * r * W * r * C
    if G.dtype != torch.float32 or G.numel() < n or (X is not None and X.numel() < n) or out.numel() < n or \
            (out_f32 is not None and (out_f32.dtype != torch.float32 or out_f32.numel() < n)):
        raise ValueError("act_grad_punshuf: a buffer is smaller than the image, or not fp32 where it must be")
    check(lib().kair_act_grad_punshuf(ptr(G), ptr(X), dtype_code(X) if X is not None else F32, ptr(out), dtype_code(out),
                                      ptr(out_f32), B, H, W, C, r, kind, slope, stream_ptr()), "act_grad_punshuf")


def axpby_rows(y, ldy, x, ldx, M, C, a, b):
    """y[:, :C] = a * x[:, :C] + b * y[:, :C] over strided fp32 rows."""
    check(lib().kair_axpby_rows(ptr(y), ldy, ptr(x), ldx, M, C, a, b, stream_ptr()), "axpby_rows")


# ------------------------------------------------------------------------------------------
# USRNet (network_usrnet_v1.py): complex planes are fp32 tensors holding float2 [planes][W][H]
# ------------------------------------------------------------------------------------------
def usr_fft_rows(src, mode, C, ld, kh, kw, sf, T, planes, Hh, Ww):
    check(lib().kair_usr_fft_rows(ptr(src), mode, C, ld, kh, kw, sf, ptr(T), planes, Hh, Ww, stream_ptr()), "usr_fft_rows")


def usr_fft_cols(mode, T, Tout, FB, FBFy, FR, invW, alpha, alpha_stride, part, planes, C, Hh, Ww, sf):
    check(lib().kair_usr_fft_cols(mode, ptr(T), ptr(Tout), ptr(FB), ptr(FBFy), ptr(FR), ptr(invW), ptr(alpha),
                                  alpha_stride, ptr(part), planes, C, Hh, Ww, sf, stream_ptr()), "usr_fft_cols")


def usr_ifft_rows(T, dst, nhwc, C, ld, scale, planes, Hh, Ww):
    check(lib().kair_usr_ifft_rows(ptr(T), ptr(dst), int(nhwc), dtype_code(dst), C, ld, scale, planes, Hh, Ww,
                                   stream_ptr()), "usr_ifft_rows")


def usr_seg_sum(ws, seglen, nseg, scale, out, ostride, accumulate=False):
    check(lib().kair_usr_seg_sum(ptr(ws), seglen, nseg, scale, ptr(out), ostride, int(accumulate), stream_ptr()),
          "usr_seg_sum")


def usr_chan_sum(x, ld, c, HW, B, ws, out, ostride, accumulate=False):
    check(lib().kair_usr_chan_sum(ptr(x), ld, c, HW, B, ptr(ws), ptr(out), ostride, int(accumulate), stream_ptr()),
          "usr_chan_sum")


def usr_upsample_nearest(L, out, planes, h, w, sf):
    check(lib().kair_usr_upsample_nearest(ptr(L), ptr(out), planes, h, w, sf, stream_ptr()), "usr_upsample_nearest")


def usr_pad(src, dst, mode, ldc, nb, H, W, Hp, Wp):
    """ResUNet replicate pad / crop and adjoints (kair_usr_pad); dst dtype = src dtype."""
    if src.dtype != dst.dtype:
        raise ValueError("usr_pad: src and dst dtypes differ")
    check(lib().kair_usr_pad(ptr(src), ptr(dst), dtype_code(dst), mode, ldc, nb, H, W, Hp, Wp, stream_ptr()), "usr_pad")


def usr_pack_input(x, beta, beta_stride, out, ld, B, C, HW):
    check(lib().kair_usr_pack_input(ptr(x), ptr(beta), beta_stride, ptr(out), dtype_code(out), ld, B, C, HW,
                                    stream_ptr()), "usr_pack_input")


def hypanet_fwd(sigma, sf, W1, b1, W2, b2, W3, b3, hc, no, B, ab):
    check(lib().kair_hypanet_fwd(ptr(sigma), sf, ptr(W1), ptr(b1), ptr(W2), ptr(b2), ptr(W3), ptr(b3), hc, no, B, ptr(ab),
                                 stream_ptr()), "hypanet_fwd")


def hypanet_bwd(sigma, sf, W1, b1, W2, b2, W3, b3, hc, no, B, gab, gW1, gb1, gW2, gb2, gW3, gb3, accumulate=False):
    check(lib().kair_hypanet_bwd(ptr(sigma), sf, ptr(W1), ptr(b1), ptr(W2), ptr(b2), ptr(W3), ptr(b3), hc, no, B, ptr(gab),
                                 ptr(gW1), ptr(gb1), ptr(gW2), ptr(gb2), ptr(gW3), ptr(gb3), int(accumulate),
                                 stream_ptr()), "hypanet_bwd")


def bn_ws(C):
    return lib().kair_bn_ws(C)


def bn_fwd(z, ldz, out, ldo, M, C, gamma, beta, running_mean, running_var, momentum, eps, training, mean, rstd, act,
           slope, ws):
    check(lib().kair_bn_fwd(ptr(z), ldz, ptr(out), dtype_code(out), ldo, M, C, ptr(gamma), ptr(beta), ptr(running_mean),
                            ptr(running_var), momentum, eps, int(training), ptr(mean), ptr(rstd), act, slope, ptr(ws),
                            stream_ptr()), "bn_fwd")


def bn_bwd(z, ldz, a, lda, da, ldda, dz, lddz, M, C, gamma, mean, rstd, act, slope, dgamma, dbeta, accumulate, ws):
    check(lib().kair_bn_bwd(ptr(z), ldz, ptr(a), dtype_code(a) if a is not None else F32, lda, ptr(da), ldda, ptr(dz),
                            dtype_code(dz), lddz, M, C, ptr(gamma), ptr(mean), ptr(rstd), act, slope, ptr(dgamma), ptr(dbeta),
                            int(accumulate), ptr(ws), stream_ptr()), "bn_bwd")


# ------------------------------------------------------------------------------------------
# training-patch synthesis (kair_amd/data/gpu_synth.py: one task class per wrapper family below)
# ------------------------------------------------------------------------------------------
def _rows_of(t, dtype, ncol, what):
    """(pointer, row stride) of a [B, >= ncol] parameter table; a column slice of a wider table is fine."""
    if t.dtype != dtype or t.dim() != 2 or t.shape[1] < ncol or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{what}: expected a [B, >= {ncol}] {dtype} table with unit column stride")
    return ptr(t), t.stride(0)


def _sample_rows(t, B, ncol, what, packed=False):
    """_rows_of an int32 table that has a row for each of B samples.  packed: the kernel reads the rows as int4, so the
    table is exactly [B, 4] with row stride 4 (no column slice of a wider table)."""
    pp, ps = _rows_of(t, torch.int32, ncol, what)
    if t.shape[0] < B:
        raise ValueError(f"{what}: fewer parameter rows than samples")
    if packed and (t.shape[1] != ncol or ps != ncol):
        raise ValueError(f"{what}: expected packed [B, {ncol}] rows (row stride {ncol}), not a slice of a wider table")
    return pp, ps


def _fp32(t, shape, what):
    """t is a contiguous fp32 tensor of exactly this shape."""
    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be a contiguous fp32 {tuple(shape)}")


def _images(t, what):
    """(N, C, H, W) of a contiguous fp32 image batch (the pool, or whole images)."""
    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 4:
        raise ValueError(f"{what} must be contiguous fp32 [N, C, H, W]")
    return t.shape


def synth_sr(pool, params, B, PS, sf, taps_h, taps_w, outH, outL):
    """DatasetSR batch (kair_synth_sr): params [B, 4] int32 {image, rnd_h, rnd_w, mode}, packed; outH [B, C, PS, PS],
    outL [B, C, PS // sf, PS // sf]."""
    require_device(pool, params, outH, outL)
    N, C, Hs, Ws = _images(pool, "synth_sr: pool")
    _fp32(outH, (B, C, PS, PS), "synth_sr: output")
    _fp32(outL, (B, C, PS // sf, PS // sf), "synth_sr: output")
    pp, _ = _sample_rows(params, B, 4, "synth_sr params", packed=True)
    (ih, wh), (iw, ww) = taps_h, taps_w
    check(lib().kair_synth_sr(ptr(pool), C, Hs, Ws, pp, B, PS, sf, ptr(wh), ptr(ih), ptr(ww), ptr(iw),
                              wh.shape[1], ptr(outH), ptr(outL), stream_ptr()), "synth_sr")


def synth_dn(pool, params, B, PS, sigma, seed, step, outH, outL):
    """DatasetDnCNN batch (kair_synth_dn): params as synth_sr's; outH and outL [B, C, PS, PS]."""
    require_device(pool, params, outH, outL)
    N, C, Hs, Ws = _images(pool, "synth_dn: pool")
    _fp32(outH, (B, C, PS, PS), "synth_dn: output")
    _fp32(outL, (B, C, PS, PS), "synth_dn: output")
    pp, _ = _sample_rows(params, B, 4, "synth_dn params", packed=True)
    check(lib().kair_synth_dn(ptr(pool), C, Hs, Ws, pp, B, PS, sigma, seed, step, ptr(outH), ptr(outL),
                              stream_ptr()), "synth_dn")


def synth_dn_map(pool, params, B, PS, seed, step, outH, outL, sigma_col=4):
    """FDnCNN / DRUNet batch (kair_synth_dn_map): params [B, >= 5] int32 {image, rnd_h, rnd_w, mode} plus the float32
    bits of the sample's sigma / 255 in column sigma_col; outH [B, C, PS, PS], outL [B, C + 1, PS, PS]."""
    require_device(pool, params, outH, outL)
    N, C, Hs, Ws = _images(pool, "synth_dn_map: pool")
    _fp32(outH, (B, C, PS, PS), "synth_dn_map: output")
    _fp32(outL, (B, C + 1, PS, PS), "synth_dn_map: output")
    pp, ps = _sample_rows(params, B, max(5, sigma_col + 1), "synth_dn_map params")
    check(lib().kair_synth_dn_map(ptr(pool), N, C, Hs, Ws, pp, ps, sigma_col, B, PS, seed, step, ptr(outH), ptr(outL),
                                  stream_ptr()), "synth_dn_map")


def synth_dpsr(pool, params, B, PS, sf, taps_h, taps_w, seed, step, outH, outL, sigma_col=4):
    """DatasetDPSR batch (kair_synth_dpsr): params [B, 8] int32, {image, rnd_h, rnd_w, mode} as synth_sr's, the float32
    bits of the sample's sigma / 255 in column sigma_col; the pool cropped to the scale, taps_h / taps_w synth_sr's;
    outH [B, C, PS, PS], outL [B, C + 1, PS // sf, PS // sf]."""
    require_device(pool, params, outH, outL, *taps_h, *taps_w)
    N, C, Hs, Ws = _images(pool, "synth_dpsr: pool")
    if sf not in (2, 3, 4) or PS % sf:
        raise ValueError(f"synth_dpsr: scale 2, 3 or 4 and an H_size divisible by it (got scale {sf}, H_size {PS})")
    if Hs % sf or Ws % sf or PS > Hs or PS > Ws:
        raise ValueError(f"synth_dpsr: the pool ({Hs} x {Ws}) must be cropped to the scale and hold the patch ({PS})")
    _fp32(outH, (B, C, PS, PS), "synth_dpsr: output")
    _fp32(outL, (B, C + 1, PS // sf, PS // sf), "synth_dpsr: output")
    pp, ps = _sample_rows(params, B, 8, "synth_dpsr params")
    if ps % 4 or params.data_ptr() % 16 or not 4 <= sigma_col < ps:
        raise ValueError("synth_dpsr params: 16-byte aligned rows of a multiple of 4 ints, the level column in 4 .. row")
    (ih, wh), (iw, ww) = taps_h, taps_w
    for t, n, d in ((ih, Hs // sf, torch.int32), (wh, Hs // sf, torch.float32), (iw, Ws // sf, torch.int32),
                    (ww, Ws // sf, torch.float32)):
        if t.dtype != d or t.dim() != 2 or t.shape != (n, wh.shape[1]) or not t.is_contiguous():
            raise ValueError(f"synth_dpsr: taps must be contiguous [{n}, P] {d} tables of the pool's bicubic x1/{sf}")
    check(lib().kair_synth_dpsr(ptr(pool), N, C, Hs, Ws, pp, ps, sigma_col, B, PS, sf, ptr(wh), ptr(ih), ptr(ww), ptr(iw),
                                wh.shape[1], seed, step, ptr(outH), ptr(outL), stream_ptr()), "synth_dpsr")


def synth_dn_level(pool, params, B, PS, seed, step, outH, outL, outC, sigma_col=4):
    """FFDNet batch (kair_synth_dn_level): synth_dn_map's parameter rows; outH and outL [B, C, PS, PS] (outL is
    synth_dn_map's outL[:, :C] bit for bit), the levels sigma / 255 in outC ([B] fp32, any shape of B elements)."""
    require_device(pool, params, outH, outL, outC)
    N, C, Hs, Ws = _images(pool, "synth_dn_level: pool")
    _fp32(outH, (B, C, PS, PS), "synth_dn_level: output")
    _fp32(outL, (B, C, PS, PS), "synth_dn_level: output")
    if outC.dtype != torch.float32 or not outC.is_contiguous() or outC.numel() != B:
        raise ValueError(f"synth_dn_level: outC must hold {B} contiguous fp32 levels")
    pp, ps = _sample_rows(params, B, max(5, sigma_col + 1), "synth_dn_level params")
    check(lib().kair_synth_dn_level(ptr(pool), N, C, Hs, Ws, pp, ps, sigma_col, B, PS, seed, step, ptr(outH), ptr(outL),
                                    ptr(outC), stream_ptr()), "synth_dn_level")


def usr_gauss_kernels(gpar, kpar, bank, out):
    """out [B, 1, ks, ks] <- the blur kernels of gpar [B, 3] {lambda1, lambda2, theta} and kpar [B, 4]
    {source, bank_idx, sf_k, mode_k}; bank [K, ks, ks] or None (kair_usr_gauss_kernels)."""
    require_device(gpar, kpar, bank, out)
    B, ks = out.shape[0], out.shape[-1]
    if out.dtype != torch.float32 or not out.is_contiguous() or out.shape[-2] != ks or out.numel() != B * ks * ks:
        raise ValueError("usr_gauss_kernels: out must be a contiguous fp32 [B, 1, ks, ks]")
    if gpar.shape[0] < B or kpar.shape[0] < B:
        raise ValueError("usr_gauss_kernels: fewer parameter rows than kernels")
    K = 0
    if bank is not None:
        if bank.dtype != torch.float32 or not bank.is_contiguous() or tuple(bank.shape[-2:]) != (ks, ks):
            raise ValueError("usr_gauss_kernels: bank must be a contiguous fp32 [K, ks, ks]")
        K = bank.numel() // (ks * ks)
    gp, gs = _rows_of(gpar, torch.float32, 3, "usr_gauss_kernels gpar")
    kp, kst = _rows_of(kpar, torch.int32, 4, "usr_gauss_kernels kpar")
    check(lib().kair_usr_gauss_kernels(gp, gs, kp, kst, ptr(bank), K, B, ks, ptr(out), stream_ptr()),
          "usr_gauss_kernels")


def _usr_sigma(sigma, B, what):
    if sigma is None:
        return None, 0
    if sigma.dtype != torch.float32 or sigma.dim() != 1 or sigma.shape[0] < B:
        raise ValueError(f"{what}: sigma must be an fp32 vector of B entries (a column of a wider table is fine)")
    return ptr(sigma), sigma.stride(0)


def synth_usr(pool, params, B, PS, sf, k, sigma, trunc8, seed, step, outH, outL, direct=False):
    """USRNet batch (kair_synth_usr): params [B, >= 4] int32 {image, rnd_h, rnd_w, mode}, k [B, 1, kh, kw],
    sigma fp32 [B] or None (noise off)."""
    require_device(pool, params, k, sigma, outH, outL)
    N, C, Hs, Ws = _images(pool, "synth_usr: pool")
    kh, kw = k.shape[-2:]
    if k.dtype != torch.float32 or not k.is_contiguous() or k.numel() != B * kh * kw:
        raise ValueError("synth_usr: k must be contiguous fp32 [B, 1, kh, kw]")
    _fp32(outH, (B, C, PS, PS), "synth_usr: output")
    _fp32(outL, (B, C, PS // sf, PS // sf), "synth_usr: output")
    pp, ps = _sample_rows(params, B, 4, "synth_usr params")
    sp, ss = _usr_sigma(sigma, B, "synth_usr")
    check(lib().kair_synth_usr(ptr(pool), N, C, Hs, Ws, pp, ps, B, PS, sf, ptr(k), kh, kw, sp, ss, int(trunc8), seed, step,
                               ptr(outH), ptr(outL), int(direct), stream_ptr()), "synth_usr")


def usr_degrade(x, k, sf, sigma, trunc8, seed, step, outL, direct=False):
    """L of whole images x [N, C, Hs, Ws] (kair_usr_degrade): k [N, 1, kh, kw] or one [kh, kw] kernel for all."""
    require_device(x, k, sigma, outL)
    N, C, Hs, Ws = _images(x, "usr_degrade: x")
    kh, kw = k.shape[-2:]
    if k.dtype != torch.float32 or not k.is_contiguous() or k.numel() not in (kh * kw, N * kh * kw):
        raise ValueError("usr_degrade: k must be contiguous fp32 [N, 1, kh, kw] or [kh, kw]")
    _fp32(outL, (N, C, -(-Hs // sf), -(-Ws // sf)), "usr_degrade: output")
    sp, ss = _usr_sigma(sigma, N, "usr_degrade")
    kstride = 0 if k.numel() == kh * kw else kh * kw
    check(lib().kair_usr_degrade(ptr(x), N, C, Hs, Ws, sf, ptr(k), kstride, kh, kw, sp, ss, int(trunc8), seed, step,
                                 ptr(outL), int(direct), stream_ptr()), "usr_degrade")


def srmd_kernels(kpar, P, out_k, out_code):
    """out_k [B, 1, 15, 15] and out_code [B, ncode] <- the anisotropic Gaussian kernels of kpar [B, >= 3] fp32 {theta,
    l1, l2} and their codes P @ vec_F(k), P [ncode, 225] fp32 (kair_srmd_kernels)."""
    require_device(kpar, P, out_k, out_code)
    B = out_k.shape[0]
    _fp32(out_k, (B, 1, 15, 15), "srmd_kernels: out_k")
    if P.dtype != torch.float32 or not P.is_contiguous() or P.dim() != 2 or P.shape[1] != 225:
        raise ValueError("srmd_kernels: P must be a contiguous fp32 [ncode, 225]")
    _fp32(out_code, (B, P.shape[0]), "srmd_kernels: out_code")
    if kpar.shape[0] < B:
        raise ValueError("srmd_kernels: fewer parameter rows than kernels")
    kp, ks = _rows_of(kpar, torch.float32, 3, "srmd_kernels kpar")
    check(lib().kair_srmd_kernels(kp, ks, ptr(P), P.shape[0], B, ptr(out_k), ptr(out_code), stream_ptr()), "srmd_kernels")


def synth_srmd(pool, params, B, PS, sf, k, code, noise_channel, taps, seed, step, outH, outL, sigma_col=4):
    """SRMD batch (kair_synth_srmd): params [B, >= 5] int32 {image, rnd_h, rnd_w, mode} plus the float32 bits of the
    sample's sigma / 255 in column sigma_col; k [B, 1, 15, 15]; code [B, ncode]; taps = (indices int32, weights fp32)
    [PS // sf, P] of utils_image.bicubic_taps(PS, PS // sf, 1 / sf); outH [B, C, PS, PS], outL [B, C + ncode (+ 1 with
    noise_channel), PS // sf, PS // sf]."""
    require_device(pool, params, k, code, outH, outL, *taps)
    N, C, Hs, Ws = _images(pool, "synth_srmd: pool")
    if PS < 1 or sf < 1 or PS % sf:
        raise ValueError(f"synth_srmd: the patch size {PS} is not divisible by the scale {sf}")
    LS = PS // sf
    _fp32(k, (B, 1, 15, 15), "synth_srmd: k")
    if code.dtype != torch.float32 or not code.is_contiguous() or code.dim() != 2 or code.shape[0] != B:
        raise ValueError("synth_srmd: code must be a contiguous fp32 [B, ncode]")
    it, wt = taps
    if (it.dtype != torch.int32 or wt.dtype != torch.float32 or it.dim() != 2 or it.shape[0] != LS or
            wt.shape != it.shape or not it.is_contiguous() or not wt.is_contiguous()):
        raise ValueError(f"synth_srmd: taps must be contiguous (int32, fp32) [{LS}, P]")
    _fp32(outH, (B, C, PS, PS), "synth_srmd: output")
    _fp32(outL, (B, C + code.shape[1] + int(bool(noise_channel)), LS, LS), "synth_srmd: output")
    pp, ps = _sample_rows(params, B, max(5, sigma_col + 1), "synth_srmd params")
    check(lib().kair_synth_srmd(ptr(pool), N, C, Hs, Ws, pp, ps, sigma_col, B, PS, sf, ptr(k), ptr(code), code.shape[1],
                                int(bool(noise_channel)), ptr(wt), ptr(it), it.shape[1], seed, step, ptr(outH), ptr(outL),
                                stream_ptr()), "synth_srmd")


def jpeg_roundtrip(x, quality, out):
    """out <- the JPEG round trip of x [N, 1 or 3, H, W] fp32 in [0, 1] (kair_jpeg_roundtrip); quality: device int32,
    one entry for all samples or N entries.  Returns the error code of a refused call through RuntimeError."""
    require_device(x, quality, out)
    N, C, Hh, W = _images(x, "jpeg_roundtrip: x")
    _fp32(out, x.shape, "jpeg_roundtrip: out")
    if quality.dtype != torch.int32 or quality.dim() != 1 or quality.shape[0] not in (1, N):
        raise ValueError("jpeg_roundtrip: quality must be an int32 vector of 1 or N entries")
    qstride = 0 if quality.shape[0] == 1 else quality.stride(0)
    ws = None
    if C == 3 and W >= 5:
        nbytes = lib().kair_jpeg_workspace_bytes(N, C, Hh, W)
        if nbytes < 0:
            raise ValueError("jpeg_roundtrip: image too large")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    check(lib().kair_jpeg_roundtrip(ptr(x), N, C, Hh, W, ptr(quality), qstride, ptr(out), ptr(ws), stream_ptr()),
          "jpeg_roundtrip")


def rgb2gray8(x, mode, out):
    """out [N, 1, H, W] <- gray uint8 / 255 of x [N, 3, H, W] (kair_rgb2gray8): mode 0 rgb2ycbcr Y, mode 1 OpenCV."""
    require_device(x, out)
    N, _, Hh, W = x.shape
    _fp32(x, (N, 3, Hh, W), "rgb2gray8: x")
    _fp32(out, (N, 1, Hh, W), "rgb2gray8: out")
    check(lib().kair_rgb2gray8(ptr(x), N, Hh, W, int(mode), ptr(out), stream_ptr()), "rgb2gray8")


def synth_jpeg(pool, params, B, PS, is_color, outH, outL):
    """JPEG CAR batch (kair_synth_jpeg): params [B, >= 8] int32 {image, rnd_h, rnd_w, mode, gray_mode, quality, rh2,
    rw2}; outH / outL [B, 3 if is_color else 1, PS, PS]."""
    require_device(pool, params, outH, outL)
    N, C, Hs, Ws = _images(pool, "synth_jpeg: pool")
    for t in (outH, outL):
        _fp32(t, (B, 3 if is_color else 1, PS, PS), "synth_jpeg: output")
    pp, ps = _sample_rows(params, B, 8, "synth_jpeg params")
    check(lib().kair_synth_jpeg(ptr(pool), N, C, Hs, Ws, pp, ps, B, PS, int(bool(is_color)), ptr(outH), ptr(outL),
                                stream_ptr()), "synth_jpeg")


def _bsr_buf(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 4 or t.shape[1] != 3:
        raise ValueError(f"{what}: expected a contiguous fp32 [B, 3, Hmax, Wmax] buffer")
    return t.shape[0], t.shape[2], t.shape[3]


def bsr_crop(pool, head, B, PS, dst):
    """dst [B, 3, PS, PS] <- the augmented crops of head [B, >= 6] int32 {image, rnd_h, rnd_w, mode, lq_h, lq_w}
    (kair_bsr_crop)."""
    require_device(pool, head, dst)
    N, C, Hs, Ws = _images(pool, "bsr_crop: pool")
    _fp32(dst, (B, 3, PS, PS), "bsr_crop: dst")
    hp, hs = _sample_rows(head, B, 6, "bsr_crop head")
    check(lib().kair_bsr_crop(ptr(pool), N, C, Hs, Ws, hp, hs, B, PS, ptr(dst), stream_ptr()), "bsr_crop")


def bsr_finish(pool, head, B, PS, sf, lq, src, outL, outH):
    """outL [B, 3, lq, lq] <- the crop of the buffer src [B, 3, PS, PS] at head's (lq_h, lq_w); outH [B, 3, lq sf, lq sf]
    <- the aligned crop of the augmented pool patch (kair_bsr_finish)."""
    require_device(pool, head, src, outL, outH)
    N, C, Hs, Ws = _images(pool, "bsr_finish: pool")
    _fp32(src, (B, 3, PS, PS), "bsr_finish: src")
    _fp32(outL, (B, 3, lq, lq), "bsr_finish: output")
    _fp32(outH, (B, 3, lq * sf, lq * sf), "bsr_finish: output")
    hp, hs = _sample_rows(head, B, 6, "bsr_finish head")
    check(lib().kair_bsr_finish(ptr(pool), N, C, Hs, Ws, hp, hs, B, PS, sf, lq, ptr(src), ptr(outL), ptr(outH),
                                stream_ptr()), "bsr_finish")


def bsr_kernels(table, nslot, slot_stride, out):
    """out [nslot, B, ks_max, ks_max] <- the Gaussian kernels of the blur rows of table [B, >= (nslot - 1) slot_stride + 16]
    int32 (slot s of sample b at table[b, s * slot_stride:]); other rows' entries are left alone (kair_bsr_kernels)."""
    require_device(table, out)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 4 or out.shape[0] != nslot:
        raise ValueError("bsr_kernels: out must be a contiguous fp32 [nslot, B, ks, ks]")
    B = out.shape[1]
    if table.shape[0] < B:
        raise ValueError("bsr_kernels: fewer table rows than samples")
    tp, ts = _rows_of(table, torch.int32, (nslot - 1) * slot_stride + 16, "bsr_kernels table")
    check(lib().kair_bsr_kernels(tp, ts, slot_stride, nslot, B, ptr(out), out.shape[2] * out.shape[3], stream_ptr()),
          "bsr_kernels")


def bsr_ops(src, dst, rows, k, taps=None, seed=0, step=0, slot=0, direct=False):
    """One slot of the blind-SR program (kair_bsr_ops): src -> dst, both [B, 3, Hmax, Wmax]; rows [B, >= 16] int32;
    k [B, ks_max, ks_max] the slot's kernels; taps = (ih, wh, iw, ww, h_in, w_in), utils_image.bicubic_taps at x1/2 of
    an (h_in, w_in) image on the device, for the MATLAB resize kind."""
    require_device(src, dst, rows, k)
    B, Hmax, Wmax = _bsr_buf(src, "bsr_ops")
    if _bsr_buf(dst, "bsr_ops") != (B, Hmax, Wmax) or src.data_ptr() == dst.data_ptr():
        raise ValueError("bsr_ops: src and dst must be two buffers of one shape")
    if k.dtype != torch.float32 or not k.is_contiguous() or k.dim() != 3 or k.shape[0] < B or rows.shape[0] < B:
        raise ValueError("bsr_ops: k must be a contiguous fp32 [B, ks, ks], rows [B, >= 16]")
    rp, rs = _rows_of(rows, torch.int32, 16, "bsr_ops rows")
    tp = [None, None, None, None, 0, 0, 0]
    if taps is not None:
        ih, wh, iw, ww, th, tw = taps
        require_device(ih, wh, iw, ww)
        P = ih.shape[1]
        for t, dt, n in ((ih, torch.int32, th), (wh, torch.float32, th), (iw, torch.int32, tw), (ww, torch.float32, tw)):
            if t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != ((n + 1) // 2, P):
                raise ValueError("bsr_ops: taps must be contiguous [ceil(n_in / 2), P] int32 indices / fp32 weights")
        tp = [ptr(ih), ptr(wh), ptr(iw), ptr(ww), P, th, tw]
    check(lib().kair_bsr_ops(ptr(src), ptr(dst), B, Hmax, Wmax, rp, rs, ptr(k), k.shape[1] * k.shape[2], *tp, seed, step,
                             slot, int(direct), stream_ptr()), "bsr_ops")


def jpeg_roundtrip_var(x, hw, w_min, quality, out, ws=None):
    """Colour JPEG round trip of the per-sample corners of a padded batch (kair_jpeg_roundtrip_var): x, out
    [N, 3, Hmax, Wmax] (out may be x); hw [N, >= 2] int32 {h, w}; quality int32 [N] (a table column is fine), <= 0
    copies; w_min the caller's lower bound on the widths.  ws: the uint8 workspace (jpeg_var_workspace), or None."""
    require_device(x, hw, quality, out, ws)
    N, Hmax, Wmax = _bsr_buf(x, "jpeg_roundtrip_var")
    if _bsr_buf(out, "jpeg_roundtrip_var") != (N, Hmax, Wmax):
        raise ValueError("jpeg_roundtrip_var: x and out must have one shape")
    if quality.dtype != torch.int32 or quality.dim() != 1 or quality.shape[0] < N or hw.shape[0] < N:
        raise ValueError("jpeg_roundtrip_var: quality must be an int32 vector of N entries, hw [N, >= 2]")
    hp, hs = _rows_of(hw, torch.int32, 2, "jpeg_roundtrip_var hw")
    if ws is None:
        ws = jpeg_var_workspace(N, Hmax, Wmax, x.device)
    check(lib().kair_jpeg_roundtrip_var(ptr(x), N, Hmax, Wmax, hp, hs, int(w_min), ptr(quality), quality.stride(0),
                                        ptr(out), ptr(ws), stream_ptr()), "jpeg_roundtrip_var")


def jpeg_var_workspace(N, Hmax, Wmax, device):
    nbytes = lib().kair_jpeg_workspace_bytes(N, 3, Hmax, Wmax)
    if nbytes <= 0:
        raise ValueError("jpeg_roundtrip_var: image too large")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def swin_attn_fwd(x, ldx, gamma, beta, eps, C, ln, ldln, mean, rstd, wqkv, bqkv, qkv, table, scale, O, ldo, o_ones_col,
                  lse, wproj, bproj, rowscale, rows_per_scale, out, ldout, nWin, nh, H, W, shift, w_split=False):
    """Fused LN1 -> qkv -> window attention -> proj + residual (kair_swin_attn_fwd)."""
    check(lib().kair_swin_attn_fwd(ptr(x), ldx, ptr(gamma), ptr(beta), eps, C, ptr(ln), ldln, ptr(mean), ptr(rstd),
                                   ptr(wqkv), ptr(bqkv), ptr(qkv), ptr(table), scale, ptr(O), ldo, o_ones_col, ptr(lse),
                                   ptr(wproj), ptr(bproj), ptr(rowscale), rows_per_scale, ptr(out), ldout, nWin, nh, H, W,
                                   shift, int(w_split), stream_ptr()), "swin_attn_fwd")


def swin_mlp_fwd(x, ldx, gamma, beta, eps, C, ln, ldln, mean, rstd, w1, b1, u, h, ldh, hd, w2, b2, rowscale,
                 rows_per_scale, out, ldout, M, Cp, Hp, w_split=False):
    """Fused LN2 -> fc1 + GELU -> fc2 + residual (kair_swin_mlp_fwd)."""
    check(lib().kair_swin_mlp_fwd(ptr(x), ldx, ptr(gamma), ptr(beta), eps, C, ptr(ln), ldln, ptr(mean), ptr(rstd),
                                  ptr(w1), ptr(b1), ptr(u), ptr(h), ldh, hd, ptr(w2), ptr(b2), ptr(rowscale),
                                  rows_per_scale, ptr(out), ldout, M, Cp, Hp, int(w_split), stream_ptr()), "swin_mlp_fwd")


def debug_attn_stamps(n=8192 * 8):
    """Phase stamps of the last bf16 attention backward run with KAIR_ATTN_STAMP=1 (perf only)."""
    buf = (ctypes.c_ulonglong * n)()
    check(lib().kair_debug_attn_stamps(ctypes.cast(buf, c_vp), n), "debug_attn_stamps")
    return list(buf)


def debug_x3_stamps(n=4 * 8 * 64 * 5):
    """Phase stamps of the last x3 NT ring launch run with KAIR_RING_DBG bit 8 (debug builds, perf only):
    [CTA 0..3][wave][iteration 0..63][loop top, chunk waited, barrier + DMA issued, MFMAs done, epilogue done]."""
    import numpy as np
    buf = np.zeros(n, dtype=np.uint64)
    check(lib().kair_debug_x3_stamps(ctypes.c_void_p(buf.ctypes.data), n), "debug_x3_stamps")
    return buf


def debug_fused_stamps(n=4096 * 8):
    """Phase stamps of the last fused attention half run with KAIR_ATTN_DBG bit 8 (debug builds, perf only)."""
    buf = (ctypes.c_ulonglong * n)()
    check(lib().kair_debug_fused_stamps(ctypes.cast(buf, c_vp), n), "debug_fused_stamps")
    return list(buf)


def swin_mlp_bwd_ws():
    return lib().kair_swin_mlp_bwd_ws()


def swin_mlp_bwd(dc, gd, w2t, w1t, du, x, gamma, mean, rstd, C, D, dco, rowscale, rows_per_scale, H, W, shift,
                 dgamma, dbeta, ws, M, Cp, Hp, dparam_acc=False):
    """Fused MLP-half backward (kair_swin_mlp_bwd)."""
    check(lib().kair_swin_mlp_bwd(ptr(dc), dc.shape[-1], ptr(gd), gd.shape[-1], ptr(w2t), ptr(w1t), ptr(du), du.shape[-1],
                                  ptr(x), x.shape[-1], ptr(gamma), ptr(mean), ptr(rstd), C, ptr(D), D.shape[-1], ptr(dco),
                                  dco.shape[-1], ptr(rowscale), rows_per_scale, H, W, shift, ptr(dgamma), ptr(dbeta),
                                  int(dparam_acc), ptr(ws), M, Cp, Hp, stream_ptr()), "swin_mlp_bwd")


# ------------------------------------------------------------------------------------------
# Swin-block input gradients as row GEMMs with fused consumers (rowgemm.hip, bf16)
# ------------------------------------------------------------------------------------------
def _rg_check(A, W, K):
    require_device(A, W)
    if A.dtype != torch.bfloat16 or W.dtype != torch.bfloat16:
        raise TypeError("kair rowgemm: bf16 operands only")
    if A.stride(-1) != 1 or A.shape[-1] < K:
        raise ValueError("kair rowgemm: A must be row-major with at least K columns")


def rowgemm_store(A, M, K, W, N, out):
    """out[m, :N] = bf16(A[m, :K] . W^T), W in pack kind 13 (kair_rowgemm_store)."""
    _rg_check(A, W, K)
    check(lib().kair_rowgemm_store(ptr(A), A.stride(0) if A.dim() > 1 else K, M, K, ptr(W), N, ptr(out),
                                   out.stride(0) if out.dim() > 1 else N, stream_ptr()), "rowgemm_store")


def rowgemm_gate(A, M, K, W, N, gate, out):
    """out[m, :N] = bf16((A[m, :K] . W^T) * gate[m, :N]) (kair_rowgemm_gate)."""
    _rg_check(A, W, K)
    check(lib().kair_rowgemm_gate(ptr(A), A.stride(0), M, K, ptr(W), N, ptr(gate), gate.stride(0), ptr(out),
                                  out.stride(0), stream_ptr()), "rowgemm_gate")


def rowgemm_ln_blocks(M, K):
    n = lib().kair_rowgemm_ln_blocks(M, K)
    if n < 0:
        check(-1, "rowgemm_ln_blocks")
    return n


def rowgemm_lnbwd(A, M, K, W, x, gamma, mean, rstd, C, D, part, win=(0, 0, 0, 0), copy=None):
    """D[t] += LayerNorm-backward(A . W^T) with the copy / dgamma-dbeta partials (kair_rowgemm_lnbwd)."""
    _rg_check(A, W, K)
    check(lib().kair_rowgemm_lnbwd(ptr(A), A.stride(0), M, K, ptr(W), ptr(x), x.stride(0), ptr(gamma), ptr(mean),
                                   ptr(rstd), C, ptr(D), D.stride(0), *win,
                                   ctypes.byref(copy) if copy is not None else None, ptr(part), stream_ptr()),
          "rowgemm_lnbwd")


def qkvblk_colsum_ws(nh):
    return lib().kair_qkvblk_colsum_ws(nh)


def qkvblk_colsum(dqkv, nWin, nh, hd, ws, bias_grad, accumulate=False):
    """bias_grad [3 * nh * hd] (+)= the column sums of the head-blocked dqkv [3][nWin][nh][64][32] (kair_qkvblk_colsum)."""
    if dqkv.numel() < 3 * nWin * nh * 64 * 32 or ws.numel() < qkvblk_colsum_ws(nh) or bias_grad.numel() < 3 * nh * hd:
        raise ValueError("qkvblk_colsum: a buffer is smaller than the geometry")
    check(lib().kair_qkvblk_colsum(ptr(dqkv), dtype_code(dqkv), nWin, nh, hd, ptr(ws), ptr(bias_grad), int(accumulate),
                                   stream_ptr()), "qkvblk_colsum")


def table_transpose(src, dst, R, C, accumulate=False):
    """dst [C][R] (+)= src [R][C]^T, fp32 (kair_table_transpose)."""
    if src.dtype != torch.float32 or dst.dtype != torch.float32 or src.numel() < R * C or dst.numel() < R * C:
        raise ValueError("table_transpose: fp32 tables of R * C elements")
    check(lib().kair_table_transpose(ptr(src), ptr(dst), R, C, int(accumulate), stream_ptr()), "table_transpose")


def scu_block_fwd(x, ldx, out, ldo, ln1, ln2, wqkv, bqkv, wproj, bproj, w1, b1, w2, b2, table, scale, B, H, W, C, shift):
    """SCUNet's narrow transformer Block in one launch (kair_scu_block_fwd): x / out fp32 token rows [B*H*W, ld] (out may
    be x), ln1 / ln2 the LayerNorm modules, the weights bf16 [N][K] row packs, biases and table [(2ws-1)^2][C/32] fp32."""
    M = B * H * W
    for w, shape in ((wqkv, (3 * C, C)), (wproj, (C, C)), (w1, (4 * C, C)), (w2, (C, 4 * C))):
        if w.dtype != torch.bfloat16 or tuple(w.shape) != shape or not w.is_contiguous():
            raise ValueError(f"scu_block_fwd: a weight pack is not a contiguous bf16 {shape}")
    for b, n in ((bqkv, 3 * C), (bproj, C), (b1, 4 * C), (b2, C), (ln1.weight, C), (ln1.bias, C), (ln2.weight, C),
                 (ln2.bias, C), (table, 225 * (C // 32))):
        if b.dtype != torch.float32 or b.numel() != n:
            raise ValueError("scu_block_fwd: a bias / LayerNorm / table operand has the wrong size or dtype")
    for t, ld in ((x, ldx), (out, ldo)):
        if t.dtype != torch.float32 or ld < C or t.storage_offset() + (M - 1) * ld + C > t.untyped_storage().nbytes() // 4:
            raise ValueError("scu_block_fwd: x / out rows exceed their buffer")
    check(lib().kair_scu_block_fwd(ptr(x), ldx, ptr(out), ldo, ptr(ln1.weight), ptr(ln1.bias), ptr(ln2.weight), ptr(ln2.bias),
                                   ln1.eps, ptr(wqkv), ptr(bqkv), ptr(wproj), ptr(bproj), ptr(w1), ptr(b1), ptr(w2), ptr(b2),
                                   ptr(table), scale, B, H, W, C, shift, stream_ptr()), "scu_block_fwd")
