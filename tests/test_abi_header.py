"""CPU: the binding's tables are derived from include/vivim_hip.h (vivim_amd/_lib.py: parse_header).  Checked here: the derived
layouts against the C compiler's own offsetof / sizeof of every field, the derived tables against the hand-written mirrors they
replaced (recorded below, field for field and entry for entry), the constants against the header, and that the parser refuses
what it does not understand."""
import ctypes
import os
import re
import subprocess

import pytest

from abi_cases import compiler
from conftest import ROOT
from vivim_amd import _lib

HEADER = os.path.join(ROOT, "include", "vivim_hip.h")
CLASSES = {py: getattr(_lib, py) for py in _lib.STRUCT_NAMES.values()}

# c_int32 / c_int64 are the classes ctypes also calls c_int / c_long here; a name per class keeps the records readable
_SCALARS = {ctypes.c_int32: "c_int32", ctypes.c_int64: "c_int64", ctypes.c_float: "c_float", ctypes.c_double: "c_double",
            ctypes.c_void_p: "c_void_p", ctypes.c_size_t: "c_size_t", ctypes.c_char_p: "c_char_p"}


def _tname(t):
    if t is None or t in _SCALARS:
        return _SCALARS.get(t)
    if issubclass(t, ctypes._Pointer):
        return f"POINTER({_tname(t._type_)})"
    if issubclass(t, ctypes.Array):
        return f"{_tname(t._type_)}*{t._length_}"
    return t.__name__


def _layout(cls):
    return tuple((n, getattr(cls, n).offset, getattr(cls, n).size, _tname(t)) for n, t in cls._fields_)


# ---- the mirrors this file replaced, recorded from them before they were deleted: (field, offset, size, type) per class,
# sizeof per class, the vivim_sizeof order, and (struct, extra, stream, restype) per entry point
LAYOUTS = {
    "SsmFwdParams": (
        ("batch", 0, 4, "c_int32"), ("dim", 4, 4, "c_int32"), ("seqlen", 8, 4, "c_int32"), ("dstate", 12, 4, "c_int32"),
        ("n_groups", 16, 4, "c_int32"), ("itype", 20, 4, "c_int32"), ("is_variable_B", 24, 4, "c_int32"), ("is_variable_C",
        28, 4, "c_int32"), ("delta_softplus", 32, 4, "c_int32"), ("_pad0", 36, 4, "c_int32"), ("u_batch_stride", 40, 8,
        "c_int64"), ("u_d_stride", 48, 8, "c_int64"), ("delta_batch_stride", 56, 8, "c_int64"), ("delta_d_stride", 64, 8,
        "c_int64"), ("z_batch_stride", 72, 8, "c_int64"), ("z_d_stride", 80, 8, "c_int64"), ("out_batch_stride", 88, 8,
        "c_int64"), ("out_d_stride", 96, 8, "c_int64"), ("out_z_batch_stride", 104, 8, "c_int64"), ("out_z_d_stride", 112,
        8, "c_int64"), ("A_d_stride", 120, 8, "c_int64"), ("A_dstate_stride", 128, 8, "c_int64"), ("B_batch_stride", 136, 8,
        "c_int64"), ("B_group_stride", 144, 8, "c_int64"), ("B_dstate_stride", 152, 8, "c_int64"), ("C_batch_stride", 160,
        8, "c_int64"), ("C_group_stride", 168, 8, "c_int64"), ("C_dstate_stride", 176, 8, "c_int64"), ("u", 184, 8,
        "c_void_p"), ("delta", 192, 8, "c_void_p"), ("A", 200, 8, "c_void_p"), ("B", 208, 8, "c_void_p"), ("C", 216, 8,
        "c_void_p"), ("D", 224, 8, "c_void_p"), ("delta_bias", 232, 8, "c_void_p"), ("z", 240, 8, "c_void_p"), ("out", 248,
        8, "c_void_p"), ("out_z", 256, 8, "c_void_p"), ("x", 264, 8, "c_void_p"), ("workspace", 272, 8, "c_void_p"),
        ("workspace_bytes", 280, 8, "c_int64")),
    "SsmBwdParams": (
        ("f", 0, 288, "SsmFwdParams"), ("dout_batch_stride", 288, 8, "c_int64"), ("dout_d_stride", 296, 8, "c_int64"),
        ("du_batch_stride", 304, 8, "c_int64"), ("du_d_stride", 312, 8, "c_int64"), ("ddelta_batch_stride", 320, 8,
        "c_int64"), ("ddelta_d_stride", 328, 8, "c_int64"), ("dz_batch_stride", 336, 8, "c_int64"), ("dz_d_stride", 344, 8,
        "c_int64"), ("dA_d_stride", 352, 8, "c_int64"), ("dA_dstate_stride", 360, 8, "c_int64"), ("dB_batch_stride", 368, 8,
        "c_int64"), ("dB_group_stride", 376, 8, "c_int64"), ("dB_dstate_stride", 384, 8, "c_int64"), ("dC_batch_stride",
        392, 8, "c_int64"), ("dC_group_stride", 400, 8, "c_int64"), ("dC_dstate_stride", 408, 8, "c_int64"), ("dout", 416,
        8, "c_void_p"), ("du", 424, 8, "c_void_p"), ("ddelta", 432, 8, "c_void_p"), ("dz", 440, 8, "c_void_p"), ("dA", 448,
        8, "c_void_p"), ("dB", 456, 8, "c_void_p"), ("dC", 464, 8, "c_void_p"), ("dD", 472, 8, "c_void_p"), ("ddelta_bias",
        480, 8, "c_void_p"), ("workspace", 488, 8, "c_void_p"), ("workspace_bytes", 496, 8, "c_int64")),
    "ConvFwdParams": (
        ("batch", 0, 4, "c_int32"), ("dim", 4, 4, "c_int32"), ("seqlen", 8, 4, "c_int32"), ("width", 12, 4, "c_int32"),
        ("itype", 16, 4, "c_int32"), ("wtype", 20, 4, "c_int32"), ("silu_activation", 24, 4, "c_int32"), ("_pad0", 28, 4,
        "c_int32"), ("x_batch_stride", 32, 8, "c_int64"), ("x_c_stride", 40, 8, "c_int64"), ("x_l_stride", 48, 8,
        "c_int64"), ("out_batch_stride", 56, 8, "c_int64"), ("out_c_stride", 64, 8, "c_int64"), ("out_l_stride", 72, 8,
        "c_int64"), ("weight_c_stride", 80, 8, "c_int64"), ("weight_width_stride", 88, 8, "c_int64"), ("x", 96, 8,
        "c_void_p"), ("weight", 104, 8, "c_void_p"), ("bias", 112, 8, "c_void_p"), ("out", 120, 8, "c_void_p")),
    "ConvBwdParams": (
        ("f", 0, 128, "ConvFwdParams"), ("dout_batch_stride", 128, 8, "c_int64"), ("dout_c_stride", 136, 8, "c_int64"),
        ("dout_l_stride", 144, 8, "c_int64"), ("dx_batch_stride", 152, 8, "c_int64"), ("dx_c_stride", 160, 8, "c_int64"),
        ("dx_l_stride", 168, 8, "c_int64"), ("dweight_c_stride", 176, 8, "c_int64"), ("dweight_width_stride", 184, 8,
        "c_int64"), ("dout", 192, 8, "c_void_p"), ("dx", 200, 8, "c_void_p"), ("dweight", 208, 8, "c_void_p"), ("dbias",
        216, 8, "c_void_p")),
    "DwConvParams": (
        ("batch", 0, 4, "c_int32"), ("depth", 4, 4, "c_int32"), ("height", 8, 4, "c_int32"), ("width", 12, 4, "c_int32"),
        ("channels", 16, 4, "c_int32"), ("kd", 20, 4, "c_int32"), ("itype", 24, 4, "c_int32"), ("flip", 28, 4, "c_int32"),
        ("x_batch_stride", 32, 8, "c_int64"), ("x_token_stride", 40, 8, "c_int64"), ("y_batch_stride", 48, 8, "c_int64"),
        ("y_token_stride", 56, 8, "c_int64"), ("x", 64, 8, "c_void_p"), ("wt", 72, 8, "c_void_p"), ("bias", 80, 8,
        "c_void_p"), ("y", 88, 8, "c_void_p"), ("act", 96, 4, "c_int32"), ("_pad1", 100, 4, "c_int32"), ("aux", 104, 8,
        "c_void_p"), ("aux_batch_stride", 112, 8, "c_int64"), ("aux_token_stride", 120, 8, "c_int64")),
    "DwConvWgradParams": (
        ("batch", 0, 4, "c_int32"), ("depth", 4, 4, "c_int32"), ("height", 8, 4, "c_int32"), ("width", 12, 4, "c_int32"),
        ("channels", 16, 4, "c_int32"), ("kd", 20, 4, "c_int32"), ("itype", 24, 4, "c_int32"), ("_pad0", 28, 4, "c_int32"),
        ("x_batch_stride", 32, 8, "c_int64"), ("x_token_stride", 40, 8, "c_int64"), ("dy_batch_stride", 48, 8, "c_int64"),
        ("dy_token_stride", 56, 8, "c_int64"), ("x", 64, 8, "c_void_p"), ("dy", 72, 8, "c_void_p"), ("dwt", 80, 8,
        "c_void_p"), ("dbias", 88, 8, "c_void_p")),
    "DirParams": (
        ("batch", 0, 4, "c_int32"), ("channels", 4, 4, "c_int32"), ("seqlen", 8, 4, "c_int32"), ("nframes", 12, 4,
        "c_int32"), ("csplit", 16, 4, "c_int32"), ("itype", 20, 4, "c_int32"), ("scale", 24, 4, "c_float"), ("_pad0", 28, 4,
        "c_int32"), ("flat_batch_stride", 32, 8, "c_int64"), ("flat_c_stride", 40, 8, "c_int64"), ("stk_batch_stride", 48,
        8, "c_int64"), ("stk_half_stride", 56, 8, "c_int64"), ("stk_dir_stride", 64, 8, "c_int64"), ("stk_c_stride", 72, 8,
        "c_int64"), ("src", 80, 8, "c_void_p"), ("dst", 88, 8, "c_void_p")),
    "ConvUpdateParams": (
        ("batch", 0, 4, "c_int32"), ("dim", 4, 4, "c_int32"), ("width", 8, 4, "c_int32"), ("itype", 12, 4, "c_int32"),
        ("wtype", 16, 4, "c_int32"), ("silu_activation", 20, 4, "c_int32"), ("x_batch_stride", 24, 8, "c_int64"),
        ("x_c_stride", 32, 8, "c_int64"), ("state_batch_stride", 40, 8, "c_int64"), ("state_c_stride", 48, 8, "c_int64"),
        ("state_w_stride", 56, 8, "c_int64"), ("weight_c_stride", 64, 8, "c_int64"), ("weight_width_stride", 72, 8,
        "c_int64"), ("out_batch_stride", 80, 8, "c_int64"), ("out_c_stride", 88, 8, "c_int64"), ("x", 96, 8, "c_void_p"),
        ("conv_state", 104, 8, "c_void_p"), ("weight", 112, 8, "c_void_p"), ("bias", 120, 8, "c_void_p"), ("out", 128, 8,
        "c_void_p")),
    "StateUpdateParams": (
        ("batch", 0, 4, "c_int32"), ("dim", 4, 4, "c_int32"), ("dstate", 8, 4, "c_int32"), ("itype", 12, 4, "c_int32"),
        ("stype", 16, 4, "c_int32"), ("dt_softplus", 20, 4, "c_int32"), ("state_batch_stride", 24, 8, "c_int64"),
        ("state_d_stride", 32, 8, "c_int64"), ("state_n_stride", 40, 8, "c_int64"), ("x_batch_stride", 48, 8, "c_int64"),
        ("x_d_stride", 56, 8, "c_int64"), ("dt_batch_stride", 64, 8, "c_int64"), ("dt_d_stride", 72, 8, "c_int64"),
        ("A_d_stride", 80, 8, "c_int64"), ("A_n_stride", 88, 8, "c_int64"), ("B_batch_stride", 96, 8, "c_int64"),
        ("B_n_stride", 104, 8, "c_int64"), ("C_batch_stride", 112, 8, "c_int64"), ("C_n_stride", 120, 8, "c_int64"),
        ("z_batch_stride", 128, 8, "c_int64"), ("z_d_stride", 136, 8, "c_int64"), ("out_batch_stride", 144, 8, "c_int64"),
        ("out_d_stride", 152, 8, "c_int64"), ("state", 160, 8, "c_void_p"), ("x", 168, 8, "c_void_p"), ("dt", 176, 8,
        "c_void_p"), ("A", 184, 8, "c_void_p"), ("B", 192, 8, "c_void_p"), ("C", 200, 8, "c_void_p"), ("D", 208, 8,
        "c_void_p"), ("z", 216, 8, "c_void_p"), ("dt_bias", 224, 8, "c_void_p"), ("out", 232, 8, "c_void_p")),
    "LayerNormParams": (
        ("batch", 0, 4, "c_int32"), ("seqlen", 4, 4, "c_int32"), ("channels", 8, 4, "c_int32"), ("itype", 12, 4, "c_int32"),
        ("otype", 16, 4, "c_int32"), ("eps", 20, 4, "c_float"), ("x_batch_stride", 24, 8, "c_int64"), ("x_c_stride", 32, 8,
        "c_int64"), ("y_batch_stride", 40, 8, "c_int64"), ("y_token_stride", 48, 8, "c_int64"), ("dx_batch_stride", 56, 8,
        "c_int64"), ("dx_c_stride", 64, 8, "c_int64"), ("x", 72, 8, "c_void_p"), ("weight", 80, 8, "c_void_p"), ("bias", 88,
        8, "c_void_p"), ("y", 96, 8, "c_void_p"), ("mean", 104, 8, "c_void_p"), ("rstd", 112, 8, "c_void_p"), ("dy", 120, 8,
        "c_void_p"), ("dx", 128, 8, "c_void_p"), ("dweight", 136, 8, "c_void_p"), ("dbias", 144, 8, "c_void_p"),
        ("workspace", 152, 8, "c_void_p")),
    "WgradNtParams": (
        ("groups", 0, 4, "c_int32"), ("m", 4, 4, "c_int32"), ("n", 8, 4, "c_int32"), ("k", 12, 4, "c_int32"), ("itype", 16,
        4, "c_int32"), ("_pad0", 20, 4, "c_int32"), ("a_group_stride", 24, 8, "c_int64"), ("a_row_stride", 32, 8,
        "c_int64"), ("b_group_stride", 40, 8, "c_int64"), ("b_row_stride", 48, 8, "c_int64"), ("out_group_stride", 56, 8,
        "c_int64"), ("out_row_stride", 64, 8, "c_int64"), ("a", 72, 8, "c_void_p"), ("b", 80, 8, "c_void_p"), ("out", 88, 8,
        "c_void_p")),
    "AddLayerNormParams": (
        ("batch", 0, 4, "c_int32"), ("seqlen", 4, 4, "c_int32"), ("channels", 8, 4, "c_int32"), ("itype", 12, 4, "c_int32"),
        ("btype", 16, 4, "c_int32"), ("otype", 20, 4, "c_int32"), ("eps", 24, 4, "c_float"), ("_pad0", 28, 4, "c_int32"),
        ("x_batch_stride", 32, 8, "c_int64"), ("x_c_stride", 40, 8, "c_int64"), ("x_new_batch_stride", 48, 8, "c_int64"),
        ("x_new_c_stride", 56, 8, "c_int64"), ("branch_batch_stride", 64, 8, "c_int64"), ("branch_token_stride", 72, 8,
        "c_int64"), ("y_batch_stride", 80, 8, "c_int64"), ("y_token_stride", 88, 8, "c_int64"), ("dres_batch_stride", 96, 8,
        "c_int64"), ("dres_c_stride", 104, 8, "c_int64"), ("dx_batch_stride", 112, 8, "c_int64"), ("dx_c_stride", 120, 8,
        "c_int64"), ("dbranch_batch_stride", 128, 8, "c_int64"), ("dbranch_token_stride", 136, 8, "c_int64"), ("x", 144, 8,
        "c_void_p"), ("branch", 152, 8, "c_void_p"), ("scale", 160, 8, "c_void_p"), ("weight", 168, 8, "c_void_p"), ("bias",
        176, 8, "c_void_p"), ("x_new", 184, 8, "c_void_p"), ("y", 192, 8, "c_void_p"), ("mean", 200, 8, "c_void_p"),
        ("rstd", 208, 8, "c_void_p"), ("dy", 216, 8, "c_void_p"), ("dres", 224, 8, "c_void_p"), ("dx", 232, 8, "c_void_p"),
        ("dbranch", 240, 8, "c_void_p"), ("dweight", 248, 8, "c_void_p"), ("dbias", 256, 8, "c_void_p"), ("workspace", 264,
        8, "c_void_p")),
    "SegLossParams": (
        ("batch", 0, 4, "c_int32"), ("classes", 4, 4, "c_int32"), ("pixels", 8, 4, "c_int32"), ("itype", 12, 4, "c_int32"),
        ("ttype", 16, 4, "c_int32"), ("gamma", 20, 4, "c_float"), ("focal_weight", 24, 4, "c_float"), ("tversky_weight", 28,
        4, "c_float"), ("tversky_alpha", 32, 4, "c_float"), ("tversky_beta", 36, 4, "c_float"), ("smooth", 40, 4,
        "c_float"), ("eps", 44, 4, "c_float"), ("logits_batch_stride", 48, 8, "c_int64"), ("logits_c_stride", 56, 8,
        "c_int64"), ("dlogits_batch_stride", 64, 8, "c_int64"), ("dlogits_c_stride", 72, 8, "c_int64"),
        ("target_batch_stride", 80, 8, "c_int64"), ("logits", 88, 8, "c_void_p"), ("target", 96, 8, "c_void_p"), ("alpha",
        104, 8, "c_void_p"), ("loss", 112, 8, "c_void_p"), ("coef", 120, 8, "c_void_p"), ("workspace", 128, 8, "c_void_p"),
        ("workspace_bytes", 136, 8, "c_int64"), ("grad_out", 144, 8, "c_void_p"), ("dlogits", 152, 8, "c_void_p")),
    "SegMetricsParams": (
        ("batch", 0, 4, "c_int32"), ("classes", 4, 4, "c_int32"), ("pixels", 8, 4, "c_int32"), ("itype", 12, 4, "c_int32"),
        ("ttype", 16, 4, "c_int32"), ("_pad0", 20, 4, "c_int32"), ("logits_batch_stride", 24, 8, "c_int64"),
        ("logits_c_stride", 32, 8, "c_int64"), ("target_batch_stride", 40, 8, "c_int64"), ("pred_batch_stride", 48, 8,
        "c_int64"), ("logits", 56, 8, "c_void_p"), ("target", 64, 8, "c_void_p"), ("counts", 72, 8, "c_void_p"), ("pred",
        80, 8, "c_void_p"), ("state", 88, 8, "c_void_p"), ("workspace", 96, 8, "c_void_p"), ("workspace_bytes", 104, 8,
        "c_int64")),
    "UpsampleParams": (
        ("batch", 0, 4, "c_int32"), ("channels", 4, 4, "c_int32"), ("in_h", 8, 4, "c_int32"), ("in_w", 12, 4, "c_int32"),
        ("out_h", 16, 4, "c_int32"), ("out_w", 20, 4, "c_int32"), ("itype", 24, 4, "c_int32"), ("layout", 28, 4, "c_int32"),
        ("x_batch_stride", 32, 8, "c_int64"), ("y_batch_stride", 40, 8, "c_int64"), ("x", 48, 8, "c_void_p"), ("y", 56, 8,
        "c_void_p"), ("dy", 64, 8, "c_void_p"), ("dx", 72, 8, "c_void_p")),
    "DecodeHeadParams": (
        ("struct_bytes", 0, 4, "c_int32"), ("batch", 4, 4, "c_int32"), ("hidden", 8, 4, "c_int32"), ("classes", 12, 4,
        "c_int32"), ("n_maps", 16, 4, "c_int32"), ("out_h", 20, 4, "c_int32"), ("out_w", 24, 4, "c_int32"), ("itype", 28, 4,
        "c_int32"), ("map_h", 32, 16, "c_int32*4"), ("map_w", 48, 16, "c_int32*4"), ("map_batch_stride", 64, 32,
        "c_int64*4"), ("logits_batch_stride", 96, 8, "c_int64"), ("maps", 104, 32, "c_void_p*4"), ("bias", 136, 8,
        "c_void_p"), ("w_out", 144, 8, "c_void_p"), ("b_out", 152, 8, "c_void_p"), ("logits", 160, 8, "c_void_p")),
    "TokenLayerNormParams": (
        ("struct_bytes", 0, 4, "c_int32"), ("rows", 4, 4, "c_int32"), ("channels", 8, 4, "c_int32"), ("itype", 12, 4,
        "c_int32"), ("otype", 16, 4, "c_int32"), ("eps", 20, 4, "c_float"), ("x_row_stride", 24, 8, "c_int64"),
        ("y_row_stride", 32, 8, "c_int64"), ("dy_row_stride", 40, 8, "c_int64"), ("dx_row_stride", 48, 8, "c_int64"), ("x",
        56, 8, "c_void_p"), ("weight", 64, 8, "c_void_p"), ("bias", 72, 8, "c_void_p"), ("y", 80, 8, "c_void_p"), ("mean",
        88, 8, "c_void_p"), ("rstd", 96, 8, "c_void_p"), ("dy", 104, 8, "c_void_p"), ("dx", 112, 8, "c_void_p"), ("dweight",
        120, 8, "c_void_p"), ("dbias", 128, 8, "c_void_p"), ("workspace", 136, 8, "c_void_p")),
    "TokenAddNormParams": (
        ("struct_bytes", 0, 4, "c_int32"), ("rows", 4, 4, "c_int32"), ("channels", 8, 4, "c_int32"), ("rows_per_sample", 12,
        4, "c_int32"), ("btype", 16, 4, "c_int32"), ("rtype", 20, 4, "c_int32"), ("otype", 24, 4, "c_int32"), ("rms", 28, 4,
        "c_int32"), ("eps", 32, 4, "c_float"), ("_pad0", 36, 4, "c_int32"), ("branch_row_stride", 40, 8, "c_int64"),
        ("res_row_stride", 48, 8, "c_int64"), ("res_out_row_stride", 56, 8, "c_int64"), ("y_row_stride", 64, 8, "c_int64"),
        ("dy_row_stride", 72, 8, "c_int64"), ("dres_row_stride", 80, 8, "c_int64"), ("dres_in_row_stride", 88, 8,
        "c_int64"), ("dbranch_row_stride", 96, 8, "c_int64"), ("branch", 104, 8, "c_void_p"), ("res", 112, 8, "c_void_p"),
        ("scale", 120, 8, "c_void_p"), ("weight", 128, 8, "c_void_p"), ("bias", 136, 8, "c_void_p"), ("res_out", 144, 8,
        "c_void_p"), ("y", 152, 8, "c_void_p"), ("mean", 160, 8, "c_void_p"), ("rstd", 168, 8, "c_void_p"), ("dy", 176, 8,
        "c_void_p"), ("dres", 184, 8, "c_void_p"), ("dres_in", 192, 8, "c_void_p"), ("dbranch", 200, 8, "c_void_p"),
        ("dweight", 208, 8, "c_void_p"), ("dbias", 216, 8, "c_void_p"), ("workspace", 224, 8, "c_void_p")),
    "OptStepParams": (
        ("struct_bytes", 0, 4, "c_int32"), ("count", 4, 4, "c_int32"), ("first_tensor", 8, 4, "c_int32"), ("first_block",
        12, 4, "c_int32"), ("n_blocks", 16, 4, "c_int32"), ("total_blocks", 20, 4, "c_int32"), ("scaled", 24, 4, "c_int32"),
        ("has_max_norm", 28, 4, "c_int32"), ("max_norm", 32, 8, "c_double"), ("lr", 40, 8, "c_double"), ("beta1", 48, 8,
        "c_double"), ("beta2", 56, 8, "c_double"), ("eps", 64, 8, "c_double"), ("weight_decay", 72, 8, "c_double"),
        ("grads", 80, 8, "POINTER(c_void_p)"), ("numel", 88, 8, "POINTER(c_int64)"), ("params", 96, 8, "c_void_p"),
        ("exp_avg", 104, 8, "c_void_p"), ("exp_avg_sq", 112, 8, "c_void_p"), ("block_map", 120, 8, "c_void_p"), ("state",
        128, 8, "c_void_p"), ("workspace", 136, 8, "c_void_p"), ("workspace_bytes", 144, 8, "c_int64")),
    "OptMwParams": (
        ("struct_bytes", 0, 4, "c_int32"), ("count", 4, 4, "c_int32"), ("first_tensor", 8, 4, "c_int32"), ("first_block",
        12, 4, "c_int32"), ("n_blocks", 16, 4, "c_int32"), ("total_blocks", 20, 4, "c_int32"), ("scaled", 24, 4, "c_int32"),
        ("has_max_norm", 28, 4, "c_int32"), ("max_norm", 32, 8, "c_double"), ("lr", 40, 8, "c_double"), ("beta1", 48, 8,
        "c_double"), ("beta2", 56, 8, "c_double"), ("eps", 64, 8, "c_double"), ("weight_decay", 72, 8, "c_double"),
        ("grads", 80, 8, "POINTER(c_void_p)"), ("numel", 88, 8, "POINTER(c_int64)"), ("params", 96, 8, "c_void_p"),
        ("exp_avg", 104, 8, "c_void_p"), ("exp_avg_sq", 112, 8, "c_void_p"), ("block_map", 120, 8, "c_void_p"), ("state",
        128, 8, "c_void_p"), ("workspace", 136, 8, "c_void_p"), ("workspace_bytes", 144, 8, "c_int64"), ("masters", 152, 8,
        "c_void_p"), ("dtype", 160, 4, "c_int32"), ("_pad0", 164, 4, "c_int32")),
}
SIZES = {
    "SsmFwdParams": 288, "SsmBwdParams": 504, "ConvFwdParams": 128, "ConvBwdParams": 224, "DwConvParams": 128,
    "DwConvWgradParams": 96, "DirParams": 96, "ConvUpdateParams": 136, "StateUpdateParams": 240, "LayerNormParams": 160,
    "WgradNtParams": 96, "AddLayerNormParams": 272, "SegLossParams": 160, "SegMetricsParams": 112, "UpsampleParams": 80,
    "DecodeHeadParams": 168, "TokenLayerNormParams": 144, "TokenAddNormParams": 232, "OptStepParams": 152, "OptMwParams": 168}
STRUCTS = [
    "SsmFwdParams", "SsmBwdParams", "ConvFwdParams", "ConvBwdParams", "DwConvParams", "DwConvWgradParams", "DirParams",
    "ConvUpdateParams", "StateUpdateParams", "LayerNormParams", "WgradNtParams", "AddLayerNormParams", "SegLossParams",
    "SegMetricsParams", "UpsampleParams"]
ENTRIES = {
    "vivim_abi_version": (None, (), False, "c_int32"),
    "vivim_add_layernorm_bwd_workspace_bytes": ("AddLayerNormParams", (), False, "c_size_t"),
    "vivim_add_layernorm_cm_bwd": ("AddLayerNormParams", (), True, "c_int32"),
    "vivim_add_layernorm_cm_fwd": ("AddLayerNormParams", (), True, "c_int32"),
    "vivim_causal_conv1d_bwd": ("ConvBwdParams", (), True, "c_int32"),
    "vivim_causal_conv1d_bwd_det": ("ConvBwdParams", ("c_void_p", "c_size_t"), True, "c_int32"),
    "vivim_causal_conv1d_bwd_det_workspace_bytes": ("ConvFwdParams", (), False, "c_size_t"),
    "vivim_causal_conv1d_fwd": ("ConvFwdParams", (), True, "c_int32"),
    "vivim_causal_conv1d_update": ("ConvUpdateParams", (), True, "c_int32"),
    "vivim_decode_head_fwd": (None, ("POINTER(DecodeHeadParams)",), True, "c_int32"),
    "vivim_dir_gather": ("DirParams", (), True, "c_int32"),
    "vivim_dir_scatter": ("DirParams", (), True, "c_int32"),
    "vivim_dwconv_fwd": ("DwConvParams", (), True, "c_int32"),
    "vivim_dwconv_wgrad": ("DwConvWgradParams", (), True, "c_int32"),
    "vivim_dwconv_wgrad_det": ("DwConvWgradParams", ("c_void_p", "c_size_t"), True, "c_int32"),
    "vivim_dwconv_wgrad_det_workspace_bytes": ("DwConvWgradParams", (), False, "c_size_t"),
    "vivim_last_error": (None, (), False, "c_char_p"),
    "vivim_layernorm_bwd_workspace_bytes": ("LayerNormParams", (), False, "c_size_t"),
    "vivim_layernorm_cm_bwd": ("LayerNormParams", (), True, "c_int32"),
    "vivim_layernorm_cm_fwd": ("LayerNormParams", (), True, "c_int32"),
    "vivim_opt_adamw": (None, ("POINTER(OptStepParams)",), True, "c_int32"),
    "vivim_opt_adamw_mw": (None, ("POINTER(OptMwParams)",), True, "c_int32"),
    "vivim_opt_finalise": (None, ("POINTER(OptStepParams)",), True, "c_int32"),
    "vivim_opt_grad_stats": (None, ("POINTER(OptStepParams)",), True, "c_int32"),
    "vivim_opt_grad_stats_mw": (None, ("POINTER(OptMwParams)",), True, "c_int32"),
    "vivim_opt_step_workspace_bytes": (None, ("POINTER(OptStepParams)",), False, "c_size_t"),
    "vivim_scan_bwd_det_call_workspace_bytes": ("SsmBwdParams", (), False, "c_size_t"),
    "vivim_scan_bwd_det_workspace_bytes": ("SsmFwdParams", (), False, "c_size_t"),
    "vivim_scan_bwd_workspace_bytes": ("SsmFwdParams", (), False, "c_size_t"),
    "vivim_scan_chunk_len": (None, ("c_int32",), False, "c_int32"),
    "vivim_scan_ckpt_len": ("SsmFwdParams", (), False, "c_int32"),
    "vivim_scan_fwd_workspace_bytes": ("SsmFwdParams", (), False, "c_size_t"),
    "vivim_seg_loss_bwd": ("SegLossParams", (), True, "c_int32"),
    "vivim_seg_loss_fwd": ("SegLossParams", (), True, "c_int32"),
    "vivim_seg_loss_workspace_bytes": ("SegLossParams", (), False, "c_size_t"),
    "vivim_seg_metrics": ("SegMetricsParams", (), True, "c_int32"),
    "vivim_seg_metrics_workspace_bytes": ("SegMetricsParams", (), False, "c_size_t"),
    "vivim_selective_scan_bwd": ("SsmBwdParams", (), True, "c_int32"),
    "vivim_selective_scan_bwd_det": ("SsmBwdParams", ("c_void_p", "c_size_t"), True, "c_int32"),
    "vivim_selective_scan_fwd": ("SsmFwdParams", (), True, "c_int32"),
    "vivim_selective_scan_fwd_lean": ("SsmFwdParams", ("c_void_p",), True, "c_int32"),
    "vivim_selective_state_update": ("StateUpdateParams", (), True, "c_int32"),
    "vivim_set_tuning": (None, ("c_int32", "c_int32"), False, "c_int32"),
    "vivim_sizeof": (None, ("c_int32",), False, "c_size_t"),
    "vivim_token_add_norm_bwd": (None, ("POINTER(TokenAddNormParams)",), True, "c_int32"),
    "vivim_token_add_norm_bwd_workspace_bytes": (None, ("POINTER(TokenAddNormParams)",), False, "c_size_t"),
    "vivim_token_add_norm_fwd": (None, ("POINTER(TokenAddNormParams)",), True, "c_int32"),
    "vivim_token_layernorm_bwd": (None, ("POINTER(TokenLayerNormParams)",), True, "c_int32"),
    "vivim_token_layernorm_bwd_workspace_bytes": (None, ("POINTER(TokenLayerNormParams)",), False, "c_size_t"),
    "vivim_token_layernorm_fwd": (None, ("POINTER(TokenLayerNormParams)",), True, "c_int32"),
    "vivim_upsample_bilinear2d_bwd": ("UpsampleParams", (), True, "c_int32"),
    "vivim_upsample_bilinear2d_fwd": ("UpsampleParams", (), True, "c_int32"),
    "vivim_wgrad_nt": ("WgradNtParams", (), True, "c_int32"),
}


def test_the_derived_tables_equal_the_mirrors_they_replaced():
    assert list(CLASSES) == list(LAYOUTS) and len(CLASSES) == 20
    for py, cls in CLASSES.items():
        assert cls.__name__ == py and issubclass(cls, ctypes.Structure)
        assert _layout(cls) == LAYOUTS[py], py
        assert ctypes.sizeof(cls) == SIZES[py], py
    assert [c.__name__ for c in _lib.STRUCTS] == STRUCTS and all(CLASSES[n] is c for n, c in zip(STRUCTS, _lib.STRUCTS))
    assert _lib.SsmBwdParams._fields_[0] == ("f", _lib.SsmFwdParams)            # by value, and the derived class itself
    assert _lib.ConvBwdParams._fields_[0] == ("f", _lib.ConvFwdParams)
    got = {name: (_tname(e.struct), tuple(_tname(t) for t in e.extra), e.stream, _tname(e.restype))
           for name, e in _lib.ENTRY_POINTS.items()}
    assert got == ENTRIES and len(got) == 53
    for e in _lib.ENTRY_POINTS.values():                                         # the classes themselves, not look-alikes
        assert e.struct is None or CLASSES[e.struct.__name__] is e.struct
        for t in e.extra:
            assert t in _SCALARS or CLASSES[t._type_.__name__] is t._type_
    assert _lib.EXPORTS == tuple(_lib.ENTRY_POINTS)


def test_layouts_match_the_c_compiler(tmp_path):
    """A C program generated from the parsed structs prints sizeof of every struct and offsetof / sizeof of every field as the
    compiler sees the header.  The field names come from the parse: a field it dropped leaves a gap in the offsets or the size,
    one it reordered or mistyped lands on another offset, one it invented does not compile."""
    cc = compiler()
    if cc is None:
        pytest.skip("no C compiler (neither cc nor the Makefile's hipcc)")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "vivim_hip.h"', "int main(void) {"]
    for c_name, py in _lib.STRUCT_NAMES.items():
        lines.append(f'    printf("{py} - %zu\\n", sizeof({c_name}));')
        for field, _ in CLASSES[py]._fields_:
            lines.append(f'    printf("{py} {field} %zu %zu\\n", offsetof({c_name}, {field}), sizeof((({c_name} *)0)->{field}));')
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(cc + ["-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    want = []
    for py, cls in CLASSES.items():
        want.append(f"{py} - {ctypes.sizeof(cls)}")
        want += [f"{py} {n} {getattr(cls, n).offset} {getattr(cls, n).size}" for n, _ in cls._fields_]
    assert out[:-1] == want and len(want) == 20 + sum(len(c._fields_) for c in CLASSES.values())
    # The header pads explicitly (_pad0, _pad1), so with the compiler's offsets confirmed every field begins where the one
    # before it ends.  A hole means the parse lost a field that alignment happened to absorb (or a new struct wants its pad).
    for cls in CLASSES.values():
        end = 0
        for n, _ in cls._fields_:
            assert getattr(cls, n).offset == end, (cls.__name__, n)
            end += getattr(cls, n).size
        assert ctypes.sizeof(cls) == end, cls.__name__


def test_constants_come_from_the_header():
    text = open(HEADER).read()

    def define(name):
        return int(re.search(rf"^#define {name} (\d+)", text, flags=re.M)[1])

    assert _lib.ABI_VERSION == define("VIVIM_ABI_VERSION") == 8
    assert _lib.OPT_CHUNK == define("VIVIM_OPT_CHUNK") and _lib.OPT_MAX_TENSORS == define("VIVIM_OPT_MAX_TENSORS")
    assert _lib.OPT_STATE_WORDS == define("VIVIM_OPT_STATE_WORDS")
    codes = dict(re.findall(r"\bVIVIM_(B?F\d\d) = (\d)", re.search(r"typedef enum \{(.*?)\} vivim_dtype_t;", text)[1]))
    assert (_lib.F32, _lib.F16, _lib.BF16) == (int(codes["F32"]), int(codes["F16"]), int(codes["BF16"])) == (0, 1, 2)
    fields = dict(_lib.OptStepParams._fields_)                       # what optimizer.py casts its host arrays into
    assert fields["grads"] is ctypes.POINTER(_lib.vp) and fields["numel"] is ctypes.POINTER(_lib.i64)
    assert dict(_lib.OptMwParams._fields_)["grads"] is ctypes.POINTER(_lib.vp)


GOOD = """
#define VIVIM_ABI_VERSION 3
typedef enum { VIVIM_F32 = 0, VIVIM_F16 = 1 } vivim_dtype_t;
typedef struct {
    int32_t n, dims[4];         /* a comment; with, punctuation */
    float eps;
    const void *a, *b;
    void *out;
} vivim_a_params;
typedef struct { int32_t struct_bytes, n; vivim_a_params f; const void *const *rows; const int64_t *numel;
                 double lr; } vivim_b_params;
int vivim_abi_version(void);
const char *vivim_last_error(void);
size_t vivim_a_bytes(const vivim_a_params *p);
int vivim_a(const vivim_a_params *p, void *ws, size_t ws_bytes, void *stream);
int vivim_b(const vivim_b_params *p, void *stream);
int vivim_tune(int which, int value);
"""
NAMES = {"vivim_a_params": "AParams", "vivim_b_params": "BParams"}


def test_the_parser_reads_what_the_header_uses():
    consts, classes, entries = _lib.parse_header(GOOD, NAMES)
    A, B = classes["AParams"], classes["BParams"]
    i32, vp = ctypes.c_int32, ctypes.c_void_p
    assert consts == {"VIVIM_ABI_VERSION": 3, "VIVIM_F32": 0, "VIVIM_F16": 1} and list(classes) == ["AParams", "BParams"]
    assert A._fields_ == [("n", i32), ("dims", i32 * 4), ("eps", ctypes.c_float), ("a", vp), ("b", vp), ("out", vp)]
    assert B._fields_ == [("struct_bytes", i32), ("n", i32), ("f", A), ("rows", ctypes.POINTER(vp)),
                          ("numel", ctypes.POINTER(ctypes.c_int64)), ("lr", ctypes.c_double)]
    E = _lib.Entry
    assert entries == {
        "vivim_abi_version": E(None, (), False, ctypes.c_int), "vivim_last_error": E(None, (), False, ctypes.c_char_p),
        "vivim_a_bytes": E(A, (), False, ctypes.c_size_t), "vivim_a": E(A, (vp, ctypes.c_size_t), True, ctypes.c_int),
        "vivim_b": E(None, (ctypes.POINTER(B),), True, ctypes.c_int),
        "vivim_tune": E(None, (ctypes.c_int, ctypes.c_int), False, ctypes.c_int)}
    assert list(entries) == re.findall(r"(vivim_\w+)\(", GOOD)                    # header order


def _struct(body):
    return GOOD.replace("float eps;", body)


@pytest.mark.parametrize("what, text, names", [
    ("an unknown field type", _struct("unsigned flags;"), NAMES),
    ("an unknown pointer type", _struct("const float *w;"), NAMES),
    ("a bit-field", _struct("int32_t flag : 1;"), NAMES),
    ("a function pointer member", _struct("void (*callback)(int);"), NAMES),
    ("a union", _struct("union { int32_t i; float f; } u;"), NAMES),
    ("a nested struct", _struct("struct { int32_t i; } s;"), NAMES),
    ("a preprocessor line inside a struct", _struct("#ifdef X\n    float eps;\n#endif"), NAMES),
    ("a struct used before it is defined", GOOD.replace("int32_t n, dims[4];", "vivim_b_params early;"), NAMES),
    ("a double argument", GOOD.replace("int vivim_tune(int which, int value);", "int vivim_tune(int which, double value);"), NAMES),
    ("an array argument", GOOD.replace("int value);", "int value[2]);"), NAMES),
    ("an unknown struct argument", GOOD.replace("(const vivim_b_params *p,", "(const vivim_c_params *p,"), NAMES),
    ("an unknown return type", GOOD.replace("size_t vivim_a_bytes", "long vivim_a_bytes"), NAMES),
    ("a conditional block of declarations", GOOD + "#if 0\nint vivim_old(int x);\n#endif\n", NAMES),
    ("a macro with arguments", GOOD + "#define VIVIM_MAX(a, b) \\\n    ((a) > (b) ? (a) : (b))\n", NAMES),
    ("something that is no declaration", GOOD + "static int counter = 0;\n", NAMES),
    ("a struct without a Python name", GOOD, {"vivim_a_params": "AParams"}),
    ("a Python name without a struct", GOOD, dict(NAMES, vivim_c_params="CParams")),
])
def test_the_parser_refuses_what_it_does_not_understand(what, text, names):
    with pytest.raises(ValueError, match="vivim_hip.h: "):
        _lib.parse_header(text, names)


def test_a_missing_header_is_an_import_error_naming_the_path(monkeypatch, tmp_path):
    gone = str(tmp_path / "include" / "vivim_hip.h")
    monkeypatch.setattr(_lib, "HEADER", gone)
    with pytest.raises(ImportError, match=re.escape(gone)):
        _lib._read_header()
