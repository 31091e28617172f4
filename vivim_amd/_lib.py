"""ctypes binding of libvivim_hip.so (C ABI: include/vivim_hip.h).

The library is the product: if it is missing or fails to load this module raises -- there is no
PyTorch/CPU fallback anywhere in vivim_amd.
"""
import collections
import ctypes
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.environ.get("VIVIM_LIB") or os.path.join(CSRC, "libvivim_hip.so")   # VIVIM_LIB: A/B builds

i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p

F32, F16, BF16 = 0, 1, 2


class SsmFwdParams(ctypes.Structure):
    _fields_ = (
        [(n, i32) for n in ("batch", "dim", "seqlen", "dstate", "n_groups", "itype", "is_variable_B",
                            "is_variable_C", "delta_softplus", "_pad0")]
        + [(n, i64) for n in ("u_batch_stride", "u_d_stride", "delta_batch_stride", "delta_d_stride",
                              "z_batch_stride", "z_d_stride", "out_batch_stride", "out_d_stride",
                              "out_z_batch_stride", "out_z_d_stride", "A_d_stride", "A_dstate_stride",
                              "B_batch_stride", "B_group_stride", "B_dstate_stride",
                              "C_batch_stride", "C_group_stride", "C_dstate_stride")]
        + [(n, vp) for n in ("u", "delta", "A", "B", "C", "D", "delta_bias", "z", "out", "out_z", "x", "workspace")]
        + [("workspace_bytes", i64)]
    )


class SsmBwdParams(ctypes.Structure):
    _fields_ = (
        [("f", SsmFwdParams)]
        + [(n, i64) for n in ("dout_batch_stride", "dout_d_stride", "du_batch_stride", "du_d_stride",
                              "ddelta_batch_stride", "ddelta_d_stride", "dz_batch_stride", "dz_d_stride",
                              "dA_d_stride", "dA_dstate_stride",
                              "dB_batch_stride", "dB_group_stride", "dB_dstate_stride",
                              "dC_batch_stride", "dC_group_stride", "dC_dstate_stride")]
        + [(n, vp) for n in ("dout", "du", "ddelta", "dz", "dA", "dB", "dC", "dD", "ddelta_bias", "workspace")]
        + [("workspace_bytes", i64)]
    )


class ConvFwdParams(ctypes.Structure):
    _fields_ = (
        [(n, i32) for n in ("batch", "dim", "seqlen", "width", "itype", "wtype", "silu_activation", "_pad0")]
        + [(n, i64) for n in ("x_batch_stride", "x_c_stride", "x_l_stride",
                              "out_batch_stride", "out_c_stride", "out_l_stride",
                              "weight_c_stride", "weight_width_stride")]
        + [(n, vp) for n in ("x", "weight", "bias", "out")]
    )


class ConvBwdParams(ctypes.Structure):
    _fields_ = (
        [("f", ConvFwdParams)]
        + [(n, i64) for n in ("dout_batch_stride", "dout_c_stride", "dout_l_stride",
                              "dx_batch_stride", "dx_c_stride", "dx_l_stride",
                              "dweight_c_stride", "dweight_width_stride")]
        + [(n, vp) for n in ("dout", "dx", "dweight", "dbias")]
    )


class DwConvParams(ctypes.Structure):
    _fields_ = (
        [(n, i32) for n in ("batch", "depth", "height", "width", "channels", "kd", "itype", "flip")]
        + [(n, i64) for n in ("x_batch_stride", "x_token_stride", "y_batch_stride", "y_token_stride")]
        + [(n, vp) for n in ("x", "wt", "bias", "y")]
        + [("act", i32), ("_pad1", i32), ("aux", vp), ("aux_batch_stride", i64), ("aux_token_stride", i64)]
    )


class DwConvWgradParams(ctypes.Structure):
    _fields_ = (
        [(n, i32) for n in ("batch", "depth", "height", "width", "channels", "kd", "itype", "_pad0")]
        + [(n, i64) for n in ("x_batch_stride", "x_token_stride", "dy_batch_stride", "dy_token_stride")]
        + [(n, vp) for n in ("x", "dy", "dwt", "dbias")]
    )


class DirParams(ctypes.Structure):
    _fields_ = ([(n, i32) for n in ("batch", "channels", "seqlen", "nframes", "csplit", "itype")]
                + [("scale", ctypes.c_float), ("_pad0", i32)]
                + [(n, i64) for n in ("flat_batch_stride", "flat_c_stride", "stk_batch_stride", "stk_half_stride",
                                      "stk_dir_stride", "stk_c_stride")]
                + [("src", vp), ("dst", vp)])


class ConvUpdateParams(ctypes.Structure):
    _fields_ = ([(n, i32) for n in ("batch", "dim", "width", "itype", "wtype", "silu_activation")]
                + [(n, i64) for n in ("x_batch_stride", "x_c_stride", "state_batch_stride", "state_c_stride",
                                      "state_w_stride", "weight_c_stride", "weight_width_stride",
                                      "out_batch_stride", "out_c_stride")]
                + [(n, vp) for n in ("x", "conv_state", "weight", "bias", "out")])


class StateUpdateParams(ctypes.Structure):
    _fields_ = ([(n, i32) for n in ("batch", "dim", "dstate", "itype", "stype", "dt_softplus")]
                + [(n, i64) for n in ("state_batch_stride", "state_d_stride", "state_n_stride", "x_batch_stride",
                                      "x_d_stride", "dt_batch_stride", "dt_d_stride", "A_d_stride", "A_n_stride",
                                      "B_batch_stride", "B_n_stride", "C_batch_stride", "C_n_stride",
                                      "z_batch_stride", "z_d_stride", "out_batch_stride", "out_d_stride")]
                + [(n, vp) for n in ("state", "x", "dt", "A", "B", "C", "D", "z", "dt_bias", "out")])


class LayerNormParams(ctypes.Structure):
    _fields_ = ([(n, i32) for n in ("batch", "seqlen", "channels", "itype", "otype")] + [("eps", ctypes.c_float)]
                + [(n, i64) for n in ("x_batch_stride", "x_c_stride", "y_batch_stride", "y_token_stride",
                                      "dx_batch_stride", "dx_c_stride")]
                + [(n, vp) for n in ("x", "weight", "bias", "y", "mean", "rstd", "dy", "dx", "dweight", "dbias", "workspace")])


class WgradNtParams(ctypes.Structure):
    _fields_ = ([(n, i32) for n in ("groups", "m", "n", "k", "itype", "_pad0")]
                + [(n, i64) for n in ("a_group_stride", "a_row_stride", "b_group_stride", "b_row_stride",
                                      "out_group_stride", "out_row_stride")]
                + [(n, vp) for n in ("a", "b", "out")])


class AddLayerNormParams(ctypes.Structure):
    _fields_ = ([(n, i32) for n in ("batch", "seqlen", "channels", "itype", "btype", "otype")]
                + [("eps", ctypes.c_float), ("_pad0", i32)]
                + [(n, i64) for n in ("x_batch_stride", "x_c_stride", "x_new_batch_stride", "x_new_c_stride",
                                      "branch_batch_stride", "branch_token_stride", "y_batch_stride", "y_token_stride",
                                      "dres_batch_stride", "dres_c_stride", "dx_batch_stride", "dx_c_stride",
                                      "dbranch_batch_stride", "dbranch_token_stride")]
                + [(n, vp) for n in ("x", "branch", "scale", "weight", "bias", "x_new", "y", "mean", "rstd", "dy", "dres",
                                     "dx", "dbranch", "dweight", "dbias", "workspace")])


class SegLossParams(ctypes.Structure):
    _fields_ = ([(n, i32) for n in ("batch", "classes", "pixels", "itype", "ttype")]
                + [(n, ctypes.c_float) for n in ("gamma", "focal_weight", "tversky_weight", "tversky_alpha", "tversky_beta",
                                                 "smooth", "eps")]
                + [(n, i64) for n in ("logits_batch_stride", "logits_c_stride", "dlogits_batch_stride", "dlogits_c_stride",
                                      "target_batch_stride")]
                + [(n, vp) for n in ("logits", "target", "alpha", "loss", "coef", "workspace")]
                + [("workspace_bytes", i64), ("grad_out", vp), ("dlogits", vp)])


class SegMetricsParams(ctypes.Structure):
    _fields_ = ([(n, i32) for n in ("batch", "classes", "pixels", "itype", "ttype", "_pad0")]
                + [(n, i64) for n in ("logits_batch_stride", "logits_c_stride", "target_batch_stride", "pred_batch_stride")]
                + [(n, vp) for n in ("logits", "target", "counts", "pred", "state", "workspace")]
                + [("workspace_bytes", i64)])


class UpsampleParams(ctypes.Structure):
    _fields_ = ([(n, i32) for n in ("batch", "channels", "in_h", "in_w", "out_h", "out_w", "itype", "layout")]
                + [("x_batch_stride", i64), ("y_batch_stride", i64)]
                + [(n, vp) for n in ("x", "y", "dy", "dx")])


class DecodeHeadParams(ctypes.Structure):
    """No vivim_sizeof row (and not in STRUCTS): the caller states its sizeof in struct_bytes and the entry point refuses
    any other value."""
    _fields_ = ([(n, i32) for n in ("struct_bytes", "batch", "hidden", "classes", "n_maps", "out_h", "out_w", "itype")]
                + [("map_h", i32 * 4), ("map_w", i32 * 4), ("map_batch_stride", i64 * 4), ("logits_batch_stride", i64),
                   ("maps", vp * 4)]
                + [(n, vp) for n in ("bias", "w_out", "b_out", "logits")])


class TokenLayerNormParams(ctypes.Structure):
    """As DecodeHeadParams: no vivim_sizeof row, not in STRUCTS, its sizeof stated in struct_bytes."""
    _fields_ = ([(n, i32) for n in ("struct_bytes", "rows", "channels", "itype", "otype")] + [("eps", ctypes.c_float)]
                + [(n, i64) for n in ("x_row_stride", "y_row_stride", "dy_row_stride", "dx_row_stride")]
                + [(n, vp) for n in ("x", "weight", "bias", "y", "mean", "rstd", "dy", "dx", "dweight", "dbias", "workspace")])


class TokenAddNormParams(ctypes.Structure):
    """As TokenLayerNormParams: no vivim_sizeof row, not in STRUCTS, its sizeof stated in struct_bytes."""
    _fields_ = ([(n, i32) for n in ("struct_bytes", "rows", "channels", "rows_per_sample", "btype", "rtype", "otype", "rms")]
                + [("eps", ctypes.c_float), ("_pad0", i32)]
                + [(n, i64) for n in ("branch_row_stride", "res_row_stride", "res_out_row_stride", "y_row_stride", "dy_row_stride",
                                      "dres_row_stride", "dres_in_row_stride", "dbranch_row_stride")]
                + [(n, vp) for n in ("branch", "res", "scale", "weight", "bias", "res_out", "y", "mean", "rstd", "dy", "dres",
                                     "dres_in", "dbranch", "dweight", "dbias", "workspace")])


OPT_CHUNK, OPT_MAX_TENSORS, OPT_STATE_WORDS = 4096, 248, 16          # VIVIM_OPT_* of the header


class OptStepParams(ctypes.Structure):
    """As TokenLayerNormParams: no vivim_sizeof row, not in STRUCTS, its sizeof stated in struct_bytes.  `grads` and `numel` are
    host arrays of `count` entries; the tables, the record and the workspace are device memory."""
    _fields_ = ([(n, i32) for n in ("struct_bytes", "count", "first_tensor", "first_block", "n_blocks", "total_blocks", "scaled",
                                    "has_max_norm")]
                + [(n, ctypes.c_double) for n in ("max_norm", "lr", "beta1", "beta2", "eps", "weight_decay")]
                + [("grads", ctypes.POINTER(vp)), ("numel", ctypes.POINTER(i64))]
                + [(n, vp) for n in ("params", "exp_avg", "exp_avg_sq", "block_map", "state", "workspace")]
                + [("workspace_bytes", i64)])


class OptMwParams(ctypes.Structure):
    """vivim_opt_mw_params: OptStepParams field for field, then the masters' table and the 16-bit type (F16 / BF16) of the call's
    parameters and gradients.  Its sizeof is stated in struct_bytes."""
    _fields_ = OptStepParams._fields_ + [("masters", vp), ("dtype", i32), ("_pad0", i32)]


# The structs in vivim_sizeof order.
STRUCTS = (SsmFwdParams, SsmBwdParams, ConvFwdParams, ConvBwdParams, DwConvParams, DwConvWgradParams, DirParams,
           ConvUpdateParams, StateUpdateParams, LayerNormParams, WgradNtParams, AddLayerNormParams, SegLossParams,
           SegMetricsParams, UpsampleParams)

# One entry per exported function: its params struct (or None), the ctypes types of the arguments between `params` and
# `stream` in the C signature, whether a stream comes last, and the restype.
Entry = collections.namedtuple("Entry", "struct extra stream restype")
_int, _size = ctypes.c_int, ctypes.c_size_t


def _kernel(struct, *extra):
    return Entry(struct, extra, True, _int)


def _query(struct, restype=_size):
    return Entry(struct, (), False, restype)


ENTRY_POINTS = {
    "vivim_abi_version": Entry(None, (), False, _int),
    "vivim_last_error": Entry(None, (), False, ctypes.c_char_p),
    "vivim_scan_chunk_len": Entry(None, (_int,), False, _int),
    "vivim_sizeof": Entry(None, (_int,), False, _size),
    "vivim_set_tuning": Entry(None, (_int, _int), False, _int),
    "vivim_scan_ckpt_len": _query(SsmFwdParams, _int),
    "vivim_scan_fwd_workspace_bytes": _query(SsmFwdParams),
    "vivim_scan_bwd_workspace_bytes": _query(SsmFwdParams),
    "vivim_selective_scan_fwd": _kernel(SsmFwdParams),
    "vivim_selective_scan_fwd_lean": _kernel(SsmFwdParams, vp),
    "vivim_selective_scan_bwd": _kernel(SsmBwdParams),
    "vivim_scan_bwd_det_workspace_bytes": _query(SsmFwdParams),
    "vivim_scan_bwd_det_call_workspace_bytes": _query(SsmBwdParams),
    "vivim_selective_scan_bwd_det": _kernel(SsmBwdParams, vp, _size),
    "vivim_causal_conv1d_fwd": _kernel(ConvFwdParams),
    "vivim_causal_conv1d_bwd": _kernel(ConvBwdParams),
    "vivim_causal_conv1d_bwd_det_workspace_bytes": _query(ConvFwdParams),
    "vivim_causal_conv1d_bwd_det": _kernel(ConvBwdParams, vp, _size),
    "vivim_dwconv_fwd": _kernel(DwConvParams),
    "vivim_dwconv_wgrad": _kernel(DwConvWgradParams),
    "vivim_dwconv_wgrad_det_workspace_bytes": _query(DwConvWgradParams),
    "vivim_dwconv_wgrad_det": _kernel(DwConvWgradParams, vp, _size),
    "vivim_dir_scatter": _kernel(DirParams),
    "vivim_dir_gather": _kernel(DirParams),
    "vivim_causal_conv1d_update": _kernel(ConvUpdateParams),
    "vivim_selective_state_update": _kernel(StateUpdateParams),
    "vivim_layernorm_cm_fwd": _kernel(LayerNormParams),
    "vivim_layernorm_cm_bwd": _kernel(LayerNormParams),
    "vivim_layernorm_bwd_workspace_bytes": _query(LayerNormParams),
    "vivim_wgrad_nt": _kernel(WgradNtParams),
    "vivim_add_layernorm_cm_fwd": _kernel(AddLayerNormParams),
    "vivim_add_layernorm_cm_bwd": _kernel(AddLayerNormParams),
    "vivim_add_layernorm_bwd_workspace_bytes": _query(AddLayerNormParams),
    "vivim_seg_loss_fwd": _kernel(SegLossParams),
    "vivim_seg_loss_bwd": _kernel(SegLossParams),
    "vivim_seg_loss_workspace_bytes": _query(SegLossParams),
    "vivim_seg_metrics": _kernel(SegMetricsParams),
    "vivim_seg_metrics_workspace_bytes": _query(SegMetricsParams),
    "vivim_upsample_bilinear2d_fwd": _kernel(UpsampleParams),
    "vivim_upsample_bilinear2d_bwd": _kernel(UpsampleParams),
    "vivim_decode_head_fwd": Entry(None, (ctypes.POINTER(DecodeHeadParams),), True, _int),
    "vivim_token_layernorm_fwd": Entry(None, (ctypes.POINTER(TokenLayerNormParams),), True, _int),
    "vivim_token_layernorm_bwd": Entry(None, (ctypes.POINTER(TokenLayerNormParams),), True, _int),
    "vivim_token_layernorm_bwd_workspace_bytes": Entry(None, (ctypes.POINTER(TokenLayerNormParams),), False, _size),
    "vivim_token_add_norm_fwd": Entry(None, (ctypes.POINTER(TokenAddNormParams),), True, _int),
    "vivim_token_add_norm_bwd": Entry(None, (ctypes.POINTER(TokenAddNormParams),), True, _int),
    "vivim_token_add_norm_bwd_workspace_bytes": Entry(None, (ctypes.POINTER(TokenAddNormParams),), False, _size),
    "vivim_opt_grad_stats": Entry(None, (ctypes.POINTER(OptStepParams),), True, _int),
    "vivim_opt_finalise": Entry(None, (ctypes.POINTER(OptStepParams),), True, _int),
    "vivim_opt_adamw": Entry(None, (ctypes.POINTER(OptStepParams),), True, _int),
    "vivim_opt_step_workspace_bytes": Entry(None, (ctypes.POINTER(OptStepParams),), False, _size),
    "vivim_opt_grad_stats_mw": Entry(None, (ctypes.POINTER(OptMwParams),), True, _int),
    "vivim_opt_adamw_mw": Entry(None, (ctypes.POINTER(OptMwParams),), True, _int),
}
EXPORTS = tuple(ENTRY_POINTS)

_lib = None


def build(force=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"])
    subprocess.check_call(["make", "-C", CSRC, "-j4"])
    return SO_PATH


def lib():
    """The loaded library; raises if it is not built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise ImportError(
                f"{SO_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C vivim_amd/csrc`). vivim_amd has no fallback path.")
        # torch is imported above, before the library: its bundled HIP runtime must be the one this process initialises --
        # loading the library (and with it /opt/rocm's libamdhip64) before `import torch` leaves two runtimes in the process
        # and every launch of ours then fails with "no ROCm-capable device is detected" (seen with build() followed by
        # smoke() in one process)
        L = ctypes.CDLL(SO_PATH)
        for name, e in ENTRY_POINTS.items():
            fn = getattr(L, name)
            fn.argtypes = ([ctypes.POINTER(e.struct)] if e.struct else []) + list(e.extra) + ([vp] if e.stream else [])
            fn.restype = e.restype
        if L.vivim_abi_version() != 8:
            raise ImportError("libvivim_hip.so ABI version mismatch")
        for which, st in enumerate(STRUCTS):
            if L.vivim_sizeof(which) != ctypes.sizeof(st):
                raise ImportError(f"struct layout mismatch for {st.__name__}: "
                                  f"C {L.vivim_sizeof(which)} vs ctypes {ctypes.sizeof(st)}")
        _lib = L
    return _lib


_ISIZE = {F32: 4, F16: 2, BF16: 2}


def algorithmic_bytes(name, P):
    """Compulsory HBM traffic of one launch: every tensor of the op read or written once
    (the checkpoint tensor x is an implementation choice and is excluded).  A `*_det` entry point
    moves the bytes of its default twin."""
    name = name.removesuffix("_det")
    f = P.f if isinstance(P, (SsmBwdParams, ConvBwdParams)) else P       # the forward half of a backward struct
    if name.startswith("vivim_opt"):                                    # g once | the slots | p, m, v read and written, g read
        if name.endswith("finalise"):
            return 8 * P.total_blocks + 4 * OPT_STATE_WORDS
        n = sum(P.numel[i] for i in range(P.count) if P.grads[i])
        if name.endswith("_mw"):                                        # a 2-byte g | master, m, v read and written, g read, p16 written
            return 2 * n + 8 * P.n_blocks if name.endswith("stats_mw") else 28 * n
        return 4 * n + 8 * P.n_blocks if name.endswith("stats") else 28 * n
    if name.startswith("vivim_add_layernorm"):
        n = P.batch * P.seqlen * P.channels
        if not P.weight:                                               # add-only: x, branch, x_new / dres, dbranch
            return n * ((2 if name.endswith("fwd") else 1) * _ISIZE[P.itype] + _ISIZE[P.btype])
        if name.endswith("fwd"):                                       # x, branch, x_new, y + mean, rstd
            return n * (2 * _ISIZE[P.itype] + _ISIZE[P.btype] + _ISIZE[P.otype]) + 8 * P.batch * P.seqlen + 8 * P.channels
        res = (_ISIZE[P.itype] if P.dres else 0) + (_ISIZE[P.otype] if P.dy else 0) + (_ISIZE[P.btype] if P.dbranch else 0)
        return n * (2 * _ISIZE[P.itype] + res) + 8 * P.batch * P.seqlen + 12 * P.channels   # x_new, dx + what is present
    if name.startswith("vivim_token_add_norm"):                         # every tensor that is given, once
        n, b, r = P.rows * P.channels, _ISIZE[P.btype], _ISIZE[P.rtype]
        stats = 8 * P.rows if P.mean and P.weight else 0
        small = (4 * (P.rows // P.rows_per_sample) if P.scale else 0) + (4 * P.channels if P.weight else 0)
        if name.endswith("fwd"):
            small += 4 * P.channels if P.weight and P.bias else 0
            return n * (b + (r if P.res else 0) + (r if P.res_out else 0) + (b if P.weight else 0)) + stats + small
        norm = bool(P.weight and P.dy)                                  # else the saved row and the statistics are not read
        small += (4 * P.channels if norm and P.dweight else 0) + (4 * P.channels if norm and P.dbias else 0)
        return (n * ((r + b if norm else 0) + (r if P.dres else 0) + (r if P.dres_in else 0) + (b if P.dbranch else 0))
                + (stats if norm else 0) + small)
    if name.startswith("vivim_token_layernorm"):                        # x, y + mean, rstd | x, dy, dx + mean, rstd, weight + dweight, dbias
        n = P.rows * P.channels
        stats = 8 * P.rows if P.mean else 0
        if name.endswith("fwd"):
            return n * (_ISIZE[P.itype] + _ISIZE[P.otype]) + stats
        return n * (2 * _ISIZE[P.itype] + _ISIZE[P.otype]) + stats + 12 * P.channels
    if name.startswith("vivim_decode_head"):                            # the maps once, the logits once, bias + w_out + b_out
        px = sum(P.map_h[s] * P.map_w[s] for s in range(P.n_maps))
        return (P.batch * (px * P.hidden + P.classes * P.out_h * P.out_w) * _ISIZE[P.itype]
                + 4 * (P.hidden + P.classes * P.hidden + P.classes))
    if name.startswith("vivim_upsample"):                               # the small and the large tensor once, either direction
        return P.batch * P.channels * (P.in_h * P.in_w + P.out_h * P.out_w) * _ISIZE[P.itype]
    if name.startswith("vivim_seg_metrics"):                            # logits, labels, the prediction map if wanted, the counts
        n = P.batch * P.pixels
        return n * (P.classes * _ISIZE[P.itype] + (8 if P.ttype == 0 else 1) + (1 if P.pred else 0)) + 12 * P.batch * P.classes
    if name.startswith("vivim_seg_loss"):                               # logits (+ dlogits), labels, the per-image factors
        n = P.batch * P.pixels
        return (n * ((2 if name.endswith("bwd") else 1) * P.classes * _ISIZE[P.itype] + (8 if P.ttype == 0 else 1))
                + 8 * P.batch * P.classes)
    if name.startswith("vivim_selective_scan"):
        s = _ISIZE[f.itype]
        act = f.batch * f.dim * f.seqlen * s
        bc = (f.batch * f.n_groups * f.dstate * f.seqlen) if f.is_variable_B else f.dim * f.dstate
        has_z = bool(f.z)
        if name.endswith("fwd_lean"):                             # u, delta, out | u, delta, z, out_z
            return (4 if has_z else 3) * act + 2 * bc * (s if f.is_variable_B else 4) + 4 * (f.dim * f.dstate + 2 * f.dim)
        if name.endswith("fwd"):
            n_act = 3 + (2 if has_z else 0)                       # u, delta, out (+ z, out_z)
            return n_act * act + 2 * bc * (s if f.is_variable_B else 4) + 4 * (f.dim * f.dstate + 2 * f.dim)
        n_act = 5 + (3 if has_z else 0) + (1 if (has_z and f.out_z) else 0)   # u, delta, dout, du, ddelta (+ z, out, dz) (+ out_z)
        return (n_act * act + 2 * bc * (s if f.is_variable_B else 4) + 2 * bc * 4
                + 4 * (2 * f.dim * f.dstate + 4 * f.dim))
    if name.endswith("_update"):
        return 0                                                       # latency-bound single-token steps: not profiled
    if name.startswith("vivim_dir"):
        return 4 * P.batch * P.channels * P.seqlen * _ISIZE[P.itype]  # one flat tensor + three stacked copies
    if name.startswith("vivim_dwconv"):
        act = P.batch * P.depth * P.height * P.width * P.channels * _ISIZE[P.itype]
        return 2 * act + 4 * P.channels * (P.kd * 9 + 1)            # x and y (or x and dy) once + taps
    if name.startswith("vivim_layernorm"):                              # x, y + mean, rstd | x, dy, dx + mean, rstd
        n = P.batch * P.seqlen * P.channels
        if name.endswith("fwd"):
            return n * (_ISIZE[P.itype] + _ISIZE[P.otype]) + 8 * P.batch * P.seqlen + 8 * P.channels
        return n * (2 * _ISIZE[P.itype] + _ISIZE[P.otype]) + 8 * P.batch * P.seqlen + 12 * P.channels
    if name.startswith("vivim_wgrad"):                                  # both operands, the fp32 products
        return P.groups * ((P.m + P.n) * P.k * _ISIZE[P.itype] + 4 * P.m * P.n)
    s = _ISIZE[f.itype]
    act = f.batch * f.dim * f.seqlen * s
    if name.endswith("fwd"):
        return 2 * act + 4 * f.dim * (f.width + 1)
    return 3 * act + 8 * f.dim * (f.width + 1)


_profile = None
_event_pool = []
_PROFILED = ("vivim_selective_scan_fwd", "vivim_selective_scan_bwd", "vivim_causal_conv1d_fwd",
             "vivim_causal_conv1d_bwd")


def profile_begin(all_kernels=False):
    """Start recording one (name, algorithmic bytes, start event, end event) tuple per C-ABI call of the hot-path
    kernels (with all_kernels=True of every launching entry point, under its own name); events are recorded on the stream the kernel is launched on
    (torch's current stream) and come from a reusable pool, so the timed region pays two hipEventRecord per call."""
    global _profile
    _profile = ([], bool(all_kernels))


def profile_end():
    """Stop recording; -> list of (name, bytes, seconds) after synchronising the recorded events."""
    global _profile
    rec = _profile[0] if _profile else []
    _profile = None
    out = []
    for name, nbytes, e0, e1 in rec:
        e1.synchronize()
        out.append((name, nbytes, e0.elapsed_time(e1) * 1e-3))
        _event_pool.extend((e0, e1))
    return out


def _event():
    if _event_pool:
        return _event_pool.pop()
    return torch.cuda.Event(enable_timing=True)


# ---- VIVIM_GUARD=1: debug mode that brackets every buffer the wrappers allocate for a kernel to write with canary
# bytes and verifies them (device sync) after each launch -- finds out-of-bounds writes without waiting for a fault.
GUARD = os.environ.get("VIVIM_GUARD", "0") not in ("0", "")
_GUARD_BYTES = 1 << 16
_guards = []


def _guarded_storage(nbytes, device):
    buf = torch.full((nbytes + 2 * _GUARD_BYTES,), 0xA5, dtype=torch.uint8, device=device)
    _guards.append(buf)
    return buf[_GUARD_BYTES:_GUARD_BYTES + nbytes]


def empty(shape, dtype, device):
    """torch.empty, or its canary-bracketed twin under VIVIM_GUARD=1."""
    if not GUARD:
        return torch.empty(shape, dtype=dtype, device=device)
    n = 1
    for d in shape:
        n *= d
    return _guarded_storage(n * torch.empty((), dtype=dtype).element_size(), device).view(dtype).view(shape)


def zeros(n, device):
    """A zeroed fp32 accumulator of n elements (dA / dB / dC / dD / dbias, dweight / dbias of the convolutions: what the
    kernels ADD into), or its canary-bracketed twin under VIVIM_GUARD=1."""
    if not GUARD:
        return torch.zeros(n, dtype=torch.float32, device=device)
    return _guarded_storage(4 * n, device).view(torch.float32).zero_()


def empty_like(t):
    """torch.empty_like (dense, same strides), or its canary-bracketed twin under VIVIM_GUARD=1."""
    if not GUARD:
        return torch.empty_like(t)
    ref = torch.empty_like(t)                               # for its strides
    flat = _guarded_storage(t.numel() * t.element_size(), t.device).view(t.dtype)
    return flat.as_strided(ref.shape, ref.stride())


def check_guards(what):
    torch.cuda.synchronize()
    for buf in _guards:
        lo, hi = buf[:_GUARD_BYTES], buf[-_GUARD_BYTES:]
        if not (bool((lo == 0xA5).all()) and bool((hi == 0xA5).all())):
            nlo, nhi = int((lo != 0xA5).sum()), int((hi != 0xA5).sum())
            _guards.clear()
            raise RuntimeError(f"VIVIM_GUARD: {what} wrote outside a {buf.numel() - 2 * _GUARD_BYTES}-byte buffer "
                               f"({nlo} bytes below, {nhi} bytes above)")
    _guards.clear()


def deterministic():
    """True while torch.use_deterministic_algorithms is on (warn_only included): the backward entry points then take
    their deterministic variants."""
    return torch.are_deterministic_algorithms_enabled()


def call(name, params, stream, *extra):
    """Enqueue one entry point on `stream` (int hipStream_t): fn(&params, *extra, stream), `extra` being what the C
    signature has between the two (ENTRY_POINTS).  RuntimeError on a nonzero return, like the TORCH_CHECKs of the
    reference bindings."""
    L = lib()
    fn = getattr(L, name)
    if _profile is not None and (_profile[1] or name in _PROFILED):
        e0, e1 = _event(), _event()
        e0.record()
        rc = fn(ctypes.byref(params), *extra, stream)
        e1.record()
        _profile[0].append((name, algorithmic_bytes(name, params), e0, e1))
    else:
        rc = fn(ctypes.byref(params), *extra, stream)
    if rc != 0:
        raise RuntimeError(L.vivim_last_error().decode())
    if GUARD:
        check_guards(name)


def launch(name, params, device, *extra):
    """`call` on torch's current stream of `device`.  The step is host-paced: the device context manager (~15 us) is
    entered only when `device` is not already the current one."""
    if device.index == torch.cuda.current_device():
        call(name, params, torch.cuda.current_stream().cuda_stream, *extra)
    else:
        with torch.cuda.device(device):
            call(name, params, torch.cuda.current_stream().cuda_stream, *extra)


# ---- what every wrapper module needs around a launch
ITYPE = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}


def ptr(t):
    return None if t is None else t.data_ptr()


def check(cond, msg):
    if not cond:
        raise RuntimeError(msg)


def workspace(query, params, device):
    """-> (bytes the query `query` asks for `params`, a uint8 buffer of that size on `device` or None for 0 bytes)."""
    n = getattr(lib(), query)(params)
    return n, (empty((n,), torch.uint8, device) if n else None)
