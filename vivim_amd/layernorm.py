"""LayerNorm over the channels of a channel-major token tensor (csrc/layernorm.hip; include/vivim_hip.h:
vivim_layernorm_params) -- the two norms around the Mamba call of MambaLayer (modeling/vivim.py:155-156).

    layer_norm_cm(x, weight, bias, eps)     x: (B, L, C) VIEW of (B, C, L) memory (token stride 1), as MambaLayer builds it
                                            -> (B, L, C) contiguous, the dtype F.layer_norm would return (f32 under autocast)
The transpose the ATen path does with a copy kernel in front of its row kernel is the kernel's own read pattern here.
`supported(x, weight)` says whether the fast path applies; the caller falls back to F.layer_norm otherwise (other layouts:
the ATen kernel is already the right one for token-major rows).

The residual add in front of the norm, fused with it (the same kernel family; vivim_add_layernorm_params) -- MambaLayer's
`x + drop_path(branch)` followed by norm2, and the layer's last add (MambaLayer(fused_add_norm=True)):

    add_layer_norm_cm(x, branch, weight, bias, eps, scale=None) -> (x_new, y)
                                            x as above; branch: (B, L, C) with unit channel stride, x's dtype (or f16 / bf16 with an
                                            f32 x: the autocast case); scale: (B,) f32 per-sample DropPath factor or None
                                            x_new = x + scale[b] * branch in x's dtype and layout, y = layer_norm(x_new)
    add_cm(x, branch, scale=None) -> x_new  the add alone
`add_norm_supported(x, branch, weight)` says whether they apply; the caller keeps its composition of torch ops otherwise.

LayerNorm of TOKEN-major rows (csrc/token_layernorm.hip; vivim_token_layernorm_params) -- the norms of the SegFormer blocks:

    layer_norm_tm(x, weight, bias, eps, out_dtype=None)   x: (..., C) with unit channel stride whose leading dimensions collapse to
                                            one row stride -> x's shape, contiguous, in out_dtype (None: what F.layer_norm returns)
`tm_supported(x, weight, bias)` says whether it applies.  No atomics: it also runs under torch.use_deterministic_algorithms.

The residual add in front of a token-major norm, fused with it (the same kernels; vivim_token_add_norm_params) -- the SegFormer
blocks' `hidden = drop_path(branch) + residual` followed by a LayerNorm (Vivim(fused_backbone_add_norm=True)):

    add_layer_norm_tm(res, branch, weight, bias, eps, scale=None, out_dtype=None, rms=False) -> (res_new, y)
                                            res, branch: (..., C) rows as above, branch in res's dtype or f16 / bf16 on an f32 res;
                                            scale: (res.shape[0],) f32 per-sample DropPath factor or None
                                            res_new = res + scale * branch, contiguous, in res's dtype; y = the norm of res_new AS
                                            STORED, in branch's dtype (out_dtype, when given, must say the same); rms: RMSNorm
    add_tm(res, branch, scale=None) -> res_new                          the add alone
    rms_norm_tm(x, weight, bias=None, eps, out_dtype=None) -> y         RMSNorm of rows, in x's dtype
`tm_add_supported(res, branch, weight, bias)` says whether they apply, `tm_add_worthwhile(res)` whether they pay."""
import ctypes

import torch

from . import _lib
from ._lib import ITYPE, ptr


def supported(x, weight):
    # under torch.use_deterministic_algorithms the caller's ATen path runs instead: the backward kernel adds its row
    # groups into dweight / dbias with float atomics
    if _lib.deterministic():
        return False
    if not (x.is_cuda and x.dim() == 3 and x.dtype in ITYPE and weight is not None and weight.dtype == torch.float32):
        return False
    B, L, C = x.shape
    e = 16 // x.element_size()
    return (x.stride(1) == 1 and C <= 512 and L % e == 0 and x.stride(0) % e == 0 and x.stride(2) % e == 0
            and x.data_ptr() % 16 == 0 and x.stride(2) >= L)


def worthwhile(x):
    """Where the fused kernels beat the ATen path on the GPU AND repay the extra host time of a Python autograd node
    (profiles/r03_layernorm.log): from a few thousand tokens up -- stages 0 and 1 of the 256 x 256 configs (32 us against 184,
    28 against 75 per norm); at stages 2 and 3 (3 840 and 960 tokens) a tile per wave leaves the chip idle and ATen's row kernels
    are as fast or faster."""
    return x.shape[0] * x.shape[1] >= 4096


def _params(x, out_dtype, eps):
    B, L, C = x.shape
    P = _lib.LayerNormParams()
    P.batch, P.seqlen, P.channels, P.itype, P.otype, P.eps = B, L, C, ITYPE[x.dtype], ITYPE[out_dtype], eps
    P.x_batch_stride, P.x_c_stride = x.stride(0), x.stride(2)
    P.x = x.data_ptr()
    return P


def _norm_forward(P, x, weight, bias, out_dtype):
    """The norm's side of a forward call (the same fields in both structs): a fresh y and the mean / rstd pair."""
    B, L, C = x.shape
    y = _lib.empty((B, L, C), out_dtype, x.device)
    stats = _lib.empty((2, B, L), torch.float32, x.device)                  # mean, rstd
    P.y_batch_stride, P.y_token_stride = L * C, C
    P.weight, P.bias = weight.data_ptr(), ptr(bias)
    P.y, P.mean = y.data_ptr(), stats.data_ptr()
    P.rstd = P.mean + 4 * B * L
    return y, stats


def _norm_backward(P, query, dy, weight, stats, out_dtype, has_bias):
    """The norm's side of a backward call (P has its sizes and types): weight, mean / rstd and, where dy arrives, dy in the
    kernel's dtype and layout, zeroed dweight / dbias and the workspace `query` sizes.  -> (dwb, what must outlive the launch)"""
    B, L, C = P.batch, P.seqlen, P.channels
    P.weight, P.mean = weight.data_ptr(), stats.data_ptr()
    P.rstd = P.mean + 4 * B * L
    if dy is None:
        return None, None
    if dy.dtype != out_dtype:
        dy = dy.to(out_dtype)
    if dy.stride(2) != 1 or dy.stride(1) < C:
        dy = dy.contiguous()
    P.dy, P.y_batch_stride, P.y_token_stride = dy.data_ptr(), dy.stride(0), dy.stride(1)
    dwb = _lib.zeros(2 * C, stats.device)                                   # dweight, dbias: one zero fill
    P.dweight = dwb.data_ptr()
    P.dbias = P.dweight + 4 * C if has_bias else None
    ws = _lib.workspace(query, P, stats.device)[1]
    P.workspace = ptr(ws)                                                   # per-tile dweight / dbias partial sums
    return dwb, (dy, ws)


class _LayerNormCM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps, out_dtype):
        P = _params(x, out_dtype, eps)
        y, stats = _norm_forward(P, x, weight, bias, out_dtype)
        _lib.launch("vivim_layernorm_cm_fwd", P, x.device)
        ctx.save_for_backward(x, weight, stats)
        ctx.eps, ctx.has_bias, ctx.out_dtype = eps, bias is not None, out_dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, stats = ctx.saved_tensors
        B, L, C = x.shape
        # dx in x's own layout: (B, C, L) memory seen as (B, L, C)
        dx = _lib.empty((B, C, L), x.dtype, x.device).transpose(1, 2)
        P = _params(x, ctx.out_dtype, ctx.eps)
        P.dx, P.dx_batch_stride, P.dx_c_stride = dx.data_ptr(), C * L, L
        dwb, _alive = _norm_backward(P, "vivim_layernorm_bwd_workspace_bytes", dy, weight, stats, ctx.out_dtype, ctx.has_bias)
        _lib.launch("vivim_layernorm_cm_bwd", P, x.device)
        return dx, dwb[:C], (dwb[C:] if ctx.has_bias else None), None, None


def layer_norm_cm(x, weight, bias, eps=1e-5, out_dtype=None):
    """F.layer_norm(x, (C,), weight, bias, eps) for a channel-major x; output dtype as ATen's under the ambient autocast state,
    or `out_dtype` (f32 or x's own: what the kernels write)."""
    if out_dtype is None:
        out_dtype = torch.float32 if torch.is_autocast_enabled() else x.dtype
    return _LayerNormCM.apply(x, weight, bias, eps, out_dtype)


def _cm_ok(t, e):
    """t: (B, L, C) view of channel-major memory the kernels can move in 16-byte vectors along the tokens."""
    return (t.stride(1) == 1 and t.shape[1] % e == 0 and t.stride(0) % e == 0 and t.stride(2) % e == 0
            and t.data_ptr() % 16 == 0 and t.stride(2) >= t.shape[1])


def add_norm_supported(x, branch, weight=None):
    """Whether add_layer_norm_cm (weight given) / add_cm (weight None) take these tensors.  False under
    torch.use_deterministic_algorithms, as `supported`: the reduce kernel adds into dweight / dbias with float atomics."""
    if _lib.deterministic():
        return False
    if not (x.is_cuda and x.dim() == 3 and x.dtype in ITYPE and branch.device == x.device and branch.shape == x.shape):
        return False
    if weight is not None and weight.dtype != torch.float32:
        return False
    if not (branch.dtype == x.dtype or (x.dtype == torch.float32 and branch.dtype in (torch.float16, torch.bfloat16))):
        return False
    C = x.shape[2]
    return C <= 512 and _cm_ok(x, 16 // x.element_size()) and branch.stride(2) == 1 and branch.stride(1) >= C


def _add_params(x, branch, scale):
    B, L, C = x.shape
    P = _lib.AddLayerNormParams()
    P.batch, P.seqlen, P.channels, P.itype, P.btype, P.otype = B, L, C, ITYPE[x.dtype], ITYPE[branch.dtype], ITYPE[x.dtype]
    P.scale = ptr(scale)
    return P


def _check_scale(scale, x):
    if scale is not None and not (scale.dtype == torch.float32 and scale.shape == (x.shape[0],) and scale.is_contiguous()
                                  and scale.device == x.device):
        raise ValueError("scale must be a contiguous (batch,) float32 tensor on x's device")


def _as_cm(g, like):
    """The gradient of a channel-major tensor, in that layout and dtype (it usually arrives so: a view of the next layer's
    contiguous (B, C, ...) gradient)."""
    if g.dtype != like.dtype:
        g = g.to(like.dtype)
    if not _cm_ok(g, 16 // g.element_size()):
        g = g.transpose(1, 2).contiguous().transpose(1, 2)
    return g


def _add_forward(x, branch, scale, P):
    """The part of the forward call both ops share: x, branch and a fresh x_new in x's layout."""
    B, L, C = x.shape
    x_new = _lib.empty((B, C, L), x.dtype, x.device).transpose(1, 2)
    P.x_batch_stride, P.x_c_stride = x.stride(0), x.stride(2)
    P.x_new_batch_stride, P.x_new_c_stride = C * L, L
    P.branch_batch_stride, P.branch_token_stride = branch.stride(0), branch.stride(1)
    P.x, P.branch, P.x_new = x.data_ptr(), branch.data_ptr(), x_new.data_ptr()
    return x_new


class _AddLayerNormCM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, branch, weight, bias, scale, eps, out_dtype):
        P = _add_params(x, branch, scale)
        P.otype, P.eps = ITYPE[out_dtype], eps
        x_new = _add_forward(x, branch, scale, P)
        y, stats = _norm_forward(P, x, weight, bias, out_dtype)
        _lib.launch("vivim_add_layernorm_cm_fwd", P, x.device)
        ctx.save_for_backward(x_new, weight, stats, scale)
        ctx.eps, ctx.has_bias, ctx.out_dtype, ctx.branch_dtype = eps, bias is not None, out_dtype, branch.dtype
        ctx.set_materialize_grads(False)                                    # an unused output's gradient stays None: the kernel skips it
        return x_new, y

    @staticmethod
    def backward(ctx, dres, dy):
        if dres is None and dy is None:
            return (None,) * 7
        x_new, weight, stats, scale = ctx.saved_tensors
        B, L, C = x_new.shape
        P = _lib.AddLayerNormParams()
        P.batch, P.seqlen, P.channels, P.eps = B, L, C, ctx.eps
        P.itype, P.btype, P.otype = ITYPE[x_new.dtype], ITYPE[ctx.branch_dtype], ITYPE[ctx.out_dtype]
        P.scale = ptr(scale)
        P.x_new_batch_stride, P.x_new_c_stride = x_new.stride(0), x_new.stride(2)
        P.x_new = x_new.data_ptr()
        dwb, _alive = _norm_backward(P, "vivim_add_layernorm_bwd_workspace_bytes", dy, weight, stats, ctx.out_dtype, ctx.has_bias)
        if dres is not None:
            dres = _as_cm(dres, x_new)
            P.dres, P.dres_batch_stride, P.dres_c_stride = dres.data_ptr(), dres.stride(0), dres.stride(2)
        # dx in x's own layout, dbranch token-major
        dx = _lib.empty((B, C, L), x_new.dtype, x_new.device).transpose(1, 2)
        P.dx, P.dx_batch_stride, P.dx_c_stride = dx.data_ptr(), C * L, L
        dbranch = None
        if ctx.needs_input_grad[1]:
            dbranch = _lib.empty((B, L, C), ctx.branch_dtype, x_new.device)
            P.dbranch, P.dbranch_batch_stride, P.dbranch_token_stride = dbranch.data_ptr(), L * C, C
        _lib.launch("vivim_add_layernorm_cm_bwd", P, x_new.device)
        return (dx, dbranch, (dwb[:C] if dwb is not None else None),
                (dwb[C:] if dwb is not None and ctx.has_bias else None), None, None, None)


class _AddCM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, branch, scale):
        P = _add_params(x, branch, scale)
        x_new = _add_forward(x, branch, scale, P)
        _lib.launch("vivim_add_layernorm_cm_fwd", P, x.device)
        ctx.save_for_backward(scale)
        ctx.branch_dtype = branch.dtype
        return x_new

    @staticmethod
    def backward(ctx, dres):
        scale, = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return dres, None, None
        dres = _as_cm(dres, dres)
        B, L, C = dres.shape
        dbranch = _lib.empty((B, L, C), ctx.branch_dtype, dres.device)
        P = _lib.AddLayerNormParams()
        P.batch, P.seqlen, P.channels = B, L, C
        P.itype, P.btype, P.otype = ITYPE[dres.dtype], ITYPE[ctx.branch_dtype], ITYPE[dres.dtype]
        P.scale = ptr(scale)
        P.dres, P.dres_batch_stride, P.dres_c_stride = dres.data_ptr(), dres.stride(0), dres.stride(2)
        P.dbranch, P.dbranch_batch_stride, P.dbranch_token_stride = dbranch.data_ptr(), L * C, C
        _lib.launch("vivim_add_layernorm_cm_bwd", P, dres.device)
        return dres, dbranch, None                                           # dx is dres itself: no kernel


def add_layer_norm_cm(x, branch, weight, bias, eps=1e-5, scale=None):
    """(x + scale[:, None, None] * branch, F.layer_norm of that sum as stored) for a channel-major x and a token-major branch;
    the sum in x's dtype and layout, the norm's dtype as layer_norm_cm's."""
    _check_scale(scale, x)
    out_dtype = torch.float32 if torch.is_autocast_enabled() else x.dtype
    return _AddLayerNormCM.apply(x, branch, weight, bias, scale, eps, out_dtype)


def add_cm(x, branch, scale=None):
    """x + scale[:, None, None] * branch in x's dtype and (channel-major) layout."""
    _check_scale(scale, x)
    return _AddCM.apply(x, branch, scale)


# ---- token-major rows (csrc/token_layernorm.hip)
TM_MAX_C = 1024


def _rows(x):
    """(rows, row stride in elements) of x seen as rows of x.shape[-1] channels, or None when its leading dimensions do not
    collapse to one stride."""
    if x.dim() == 0 or x.numel() == 0:
        return None
    C = x.shape[-1]
    if x.dim() == 1:
        return 1, C
    rows, stride = x.shape[-2], x.stride(-2)
    for d in range(x.dim() - 3, -1, -1):
        if x.shape[d] == 1:
            continue
        if rows == 1:
            stride = x.stride(d)
        elif x.stride(d) != stride * rows:
            return None
        rows *= x.shape[d]
    return (rows, stride) if rows > 1 else (1, C)


def tm_pair_ok(in_dtype, out_dtype):
    """The (x, y) dtype pairs the kernels are built for: the same, an f32 output, or an f32 input (the autocast case)."""
    return in_dtype in ITYPE and out_dtype in ITYPE and (out_dtype == in_dtype or torch.float32 in (in_dtype, out_dtype))


def tm_rows(x, weight, bias=None):
    """(rows, row stride) when layer_norm_tm takes these tensors, else None."""
    if not (x.is_cuda and x.dtype in ITYPE and x.dim() >= 1 and x.stride(-1) == 1 and 1 <= x.shape[-1] <= TM_MAX_C):
        return None
    if weight is None:
        return None
    for t in (weight, bias):
        if t is not None and not (t.dtype == torch.float32 and t.device == x.device and t.shape == (x.shape[-1],)
                                  and t.is_contiguous()):
            return None
    rs = _rows(x)
    return rs if rs is not None and rs[1] >= x.shape[-1] and rs[0] < 2 ** 31 else None


def tm_supported(x, weight, bias=None):
    """Whether layer_norm_tm takes these tensors.  True under torch.use_deterministic_algorithms as well: the kernels have no
    atomics."""
    return tm_rows(x, weight, bias) is not None


def tm_worthwhile(x):
    """Where the token-major kernels repay the host time of a Python autograd node (profiles/r08_layernorm_tm.txt): from 2^21
    elements up.  The kernels of one forward + backward take 15-22 us of GPU time against ATen's 20-170 at the bench's four
    stage shapes, but back to back the call costs 71-79 us of host time against ATen's 47-62, and the train step is
    host-paced: only where ATen's own kernels take longer than that -- (61440, 64): 0.44-0.50x ATen's time per call; (15360, 128),
    1.97 M elements: 1.07-1.81x -- does the call come out ahead."""
    return x.numel() >= 1 << 21


def tm_workspace_slots(rows):
    """Slots of the backward's workspace, 2 * C floats each (include/vivim_hip.h; vivim_token_layernorm_bwd_workspace_bytes)."""
    return min(1024, (rows + 3) // 4)


class _LayerNormTM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps, out_dtype, need_stats, rs):
        rows, C = rs[0], x.shape[-1]
        P = _lib.TokenLayerNormParams()
        P.struct_bytes = ctypes.sizeof(_lib.TokenLayerNormParams)
        P.rows, P.channels, P.itype, P.otype, P.eps = rows, C, ITYPE[x.dtype], ITYPE[out_dtype], eps
        P.x, P.x_row_stride = x.data_ptr(), rs[1]
        y = _lib.empty(tuple(x.shape), out_dtype, x.device)
        P.y, P.y_row_stride = y.data_ptr(), C
        P.weight, P.bias = weight.data_ptr(), ptr(bias)
        stats = None
        if need_stats:                                                      # mean, rstd: only for a call a backward may follow
            stats = _lib.empty((2, rows), torch.float32, x.device)
            P.mean = stats.data_ptr()
            P.rstd = P.mean + 4 * rows
        _lib.launch("vivim_token_layernorm_fwd", P, x.device)
        ctx.save_for_backward(x, weight, stats)
        ctx.P, ctx.has_bias, ctx.out_dtype = P, bias is not None, out_dtype  # the backward fills in its own fields of P
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, stats = ctx.saved_tensors
        P, C = ctx.P, x.shape[-1]
        if dy.dtype != ctx.out_dtype:
            dy = dy.to(ctx.out_dtype)
        rs = _rows(dy) if dy.stride(-1) == 1 else None
        if rs is None or rs[1] < C:
            dy = dy.contiguous()
            rs = (P.rows, C)
        dx = _lib.empty(tuple(x.shape), x.dtype, x.device)
        P.dy, P.dy_row_stride, P.dx, P.dx_row_stride = dy.data_ptr(), rs[1], dx.data_ptr(), C
        need_w, need_b = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dwb = ws = None
        P.dweight = P.dbias = P.workspace = None
        if need_w or need_b:
            dwb = _lib.empty((2, C), torch.float32, x.device)               # written by the slot sum: no zero fill
            P.dweight = dwb.data_ptr() if need_w else None
            P.dbias = dwb.data_ptr() + 4 * C if need_b else None
            ws = _lib.empty((tm_workspace_slots(P.rows) * 2 * C,), torch.float32, x.device)   # one slot of partial sums per workgroup
            P.workspace = ws.data_ptr()
        _lib.launch("vivim_token_layernorm_bwd", P, x.device)
        return dx, (dwb[0] if need_w else None), (dwb[1] if need_b else None), None, None, None, None


def layer_norm_tm(x, weight, bias, eps=1e-5, out_dtype=None, rows=None):
    """F.layer_norm(x, (C,), weight, bias, eps) for token-major rows.  out_dtype None: ATen's dtype -- f32 under autocast (layer_norm
    is on its fp32 list), x's own otherwise; a 16-bit out_dtype with an f32 x is the cast the consumer's autocast would add, done
    where the value is rounded anyway.  `rows`: what tm_rows(x, weight, bias) returned, from a caller that has just asked."""
    if out_dtype is None:
        out_dtype = torch.float32 if torch.is_autocast_enabled() else x.dtype
    if rows is None:
        rows = tm_rows(x, weight, bias)
        if rows is None:
            raise ValueError("layer_norm_tm: unsupported tensors (tm_supported)")
    if not tm_pair_ok(x.dtype, out_dtype):
        raise ValueError(f"layer_norm_tm: {x.dtype} rows with a {out_dtype} output are not built")
    need_stats = torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad))
    return _LayerNormTM.apply(x, weight, bias, eps, out_dtype, need_stats, rows)


# ---- residual add + norm over token-major rows (the ADD instantiation of csrc/token_layernorm.hip)
def tm_add_pair_ok(branch_dtype, res_dtype):
    """The (branch = y, residual) dtype pairs the kernels are built for: the same, or f16 / bf16 on an f32 residual stream."""
    return branch_dtype in ITYPE and (res_dtype == branch_dtype or res_dtype == torch.float32)


def tm_add_rows(res, branch, weight=None, bias=None):
    """(rows, res's row stride, branch's row stride) when add_layer_norm_tm (weight given) / add_tm (weight None) take these
    tensors, else None."""
    if not (res.is_cuda and branch.is_cuda and res.device == branch.device and tuple(res.shape) == tuple(branch.shape)):
        return None
    if not (res.dim() >= 1 and tm_add_pair_ok(branch.dtype, res.dtype) and 1 <= res.shape[-1] <= TM_MAX_C):
        return None
    if res.stride(-1) != 1 or branch.stride(-1) != 1:
        return None
    for t in (weight, bias):
        if t is not None and not (t.dtype == torch.float32 and t.device == res.device and tuple(t.shape) == (res.shape[-1],)
                                  and t.is_contiguous()):
            return None
    a, b = _rows(res), _rows(branch)
    if a is None or b is None or min(a[1], b[1]) < res.shape[-1] or a[0] >= 2 ** 31:
        return None
    return a[0], a[1], b[1]


def tm_add_supported(res, branch, weight=None, bias=None):
    """Whether add_layer_norm_tm / add_tm take these tensors.  True under torch.use_deterministic_algorithms as well: the kernels
    have no atomics."""
    return tm_add_rows(res, branch, weight, bias) is not None


def tm_add_worthwhile(res):
    """Where the fused add + norm repays the host time of its Python autograd node: at no shape of the bench yet
    (profiles/r10_add_norm_tm.txt, five runs).  The kernels of one forward + backward take 14-32 us of GPU time against 34-203 for
    the ATen composition (mul, add, layer_norm, the consumer's cast and their backward: 8-11 launches) at the four stage shapes, but
    back to back the call is host time, 92-98 us on a quiet host and up to 237 on a busy one, whatever the shape.  With an fp32
    branch it wins at (61440, 64) in every run (0.52-0.54x) and loses below (1.12-1.24x); with the bf16 branch of the autocast step
    it is level with the composition at the three smaller shapes (0.89-0.99x; three disturbed rows at 1.04, 1.23, 1.33) and at
    (61440, 64), where the composition's own kernels take 190 us, it was 0.49x, 0.49x and 0.91x in three runs and 1.04x and 1.23x
    in the other two.  The rule is "at or below the composition in every run", and `res` is fp32 in either case: no element
    count qualifies."""
    return False


def _grad_rows(g, dtype, rows, C):
    """A gradient in the kernel's dtype, as rows of C channels with one row stride -> (g, row stride)."""
    if g.dtype != dtype:
        g = g.to(dtype)
    rs = _rows(g) if g.stride(-1) == 1 else None
    if rs is None or rs[1] < C:
        return g.contiguous(), C
    return g, rs[1]


def _add_norm_params(rows, C, branch_dtype, res_dtype, scale, eps=0.0, rms=False):
    P = _lib.TokenAddNormParams()
    P.struct_bytes = ctypes.sizeof(_lib.TokenAddNormParams)
    P.rows, P.channels, P.eps, P.rms = rows, C, eps, int(rms)
    P.btype = P.otype = ITYPE[branch_dtype]
    P.rtype = ITYPE[res_dtype]
    if scale is not None:
        P.scale, P.rows_per_sample = scale.data_ptr(), rows // scale.shape[0]
    return P


class _AddNormTM(torch.autograd.Function):
    """res may be None (h = scale * branch); `res_dtype` None then stores no sum: the norm reads the branch itself."""

    @staticmethod
    def forward(ctx, res, branch, weight, bias, scale, eps, rms, need_stats, rows, res_dtype):
        n, res_stride, branch_stride = rows
        C = branch.shape[-1]
        P = _add_norm_params(n, C, branch.dtype, res_dtype or branch.dtype, scale, eps, rms)
        P.branch, P.branch_row_stride = branch.data_ptr(), branch_stride
        if res is not None:
            P.res, P.res_row_stride = res.data_ptr(), res_stride
        res_new = None
        if res_dtype is not None:
            res_new = _lib.empty(tuple(branch.shape), res_dtype, branch.device)
            P.res_out, P.res_out_row_stride = res_new.data_ptr(), C
        y = _lib.empty(tuple(branch.shape), branch.dtype, branch.device)
        P.y, P.y_row_stride = y.data_ptr(), C
        P.weight, P.bias = weight.data_ptr(), ptr(bias)
        stats = None
        if need_stats:                                                      # mean, rstd: only for a call a backward may follow
            stats = _lib.empty((2, n), torch.float32, branch.device)
            P.mean = stats.data_ptr()
            P.rstd = P.mean + 4 * n
        _lib.launch("vivim_token_add_norm_fwd", P, branch.device)
        # the row the norm read: the stored sum, or the branch itself (its row stride then)
        ctx.save_for_backward(res_new if res_new is not None else branch, weight, stats, scale)
        ctx.h_stride = C if res_new is not None else branch_stride
        ctx.eps, ctx.rms, ctx.has_bias, ctx.branch_dtype, ctx.has_res = eps, rms, bias is not None, branch.dtype, res is not None
        ctx.set_materialize_grads(False)                                    # an unused output's gradient stays None: NULL in the struct
        return res_new, y

    @staticmethod
    def backward(ctx, dres, dy):
        if dres is None and dy is None:
            return (None,) * 10
        h, weight, stats, scale = ctx.saved_tensors
        C, n = h.shape[-1], stats.shape[1]
        P = _add_norm_params(n, C, ctx.branch_dtype, h.dtype, scale, ctx.eps, ctx.rms)
        P.res_out, P.res_out_row_stride = h.data_ptr(), ctx.h_stride
        P.weight, P.mean = weight.data_ptr(), stats.data_ptr()
        P.rstd = P.mean + 4 * n
        if dy is not None:
            dy, P.dy_row_stride = _grad_rows(dy, ctx.branch_dtype, n, C)
            P.dy = dy.data_ptr()
        if dres is not None:
            dres, P.dres_row_stride = _grad_rows(dres, h.dtype, n, C)
            P.dres = dres.data_ptr()
        need_res, need_branch = ctx.has_res and ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        # without a scale and in one dtype the two gradients are the same bits: written once
        shared = scale is None and ctx.branch_dtype == h.dtype and (need_res or need_branch)
        dres_in = dbranch = None
        if need_res or shared:
            dres_in = _lib.empty(tuple(h.shape), h.dtype, h.device)
            P.dres_in, P.dres_in_row_stride = dres_in.data_ptr(), C
        if need_branch and not shared:
            dbranch = _lib.empty(tuple(h.shape), ctx.branch_dtype, h.device)
            P.dbranch, P.dbranch_row_stride = dbranch.data_ptr(), C
        need_w = dy is not None and ctx.needs_input_grad[2]
        need_b = dy is not None and ctx.has_bias and ctx.needs_input_grad[3]
        dwb = ws = None
        if need_w or need_b:
            dwb = _lib.empty((2, C), torch.float32, h.device)               # written by the slot sum: no zero fill
            P.dweight = dwb.data_ptr() if need_w else None
            P.dbias = dwb.data_ptr() + 4 * C if need_b else None
            ws = _lib.empty((tm_workspace_slots(n) * 2 * C,), torch.float32, h.device)
            P.workspace = ws.data_ptr()
        _lib.launch("vivim_token_add_norm_bwd", P, h.device)
        if shared:
            dbranch = dres_in if need_branch else None
            dres_in = dres_in if need_res else None
        return (dres_in, dbranch, (dwb[0] if need_w else None), (dwb[1] if need_b else None)) + (None,) * 6


class _AddTM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, res, branch, scale, rows):
        n, res_stride, branch_stride = rows
        C = res.shape[-1]
        P = _add_norm_params(n, C, branch.dtype, res.dtype, scale)
        P.branch, P.branch_row_stride, P.res, P.res_row_stride = branch.data_ptr(), branch_stride, res.data_ptr(), res_stride
        res_new = _lib.empty(tuple(res.shape), res.dtype, res.device)
        P.res_out, P.res_out_row_stride = res_new.data_ptr(), C
        _lib.launch("vivim_token_add_norm_fwd", P, res.device)
        ctx.save_for_backward(scale)
        ctx.branch_dtype, ctx.n = branch.dtype, n
        return res_new

    @staticmethod
    def backward(ctx, dres):
        scale, = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return dres, None, None, None
        if scale is None and ctx.branch_dtype == dres.dtype:
            return dres, dres, None, None                                   # both gradients are dres itself: no kernel
        C = dres.shape[-1]
        g, stride = _grad_rows(dres, dres.dtype, ctx.n, C)
        P = _add_norm_params(ctx.n, C, ctx.branch_dtype, g.dtype, scale)
        P.dres, P.dres_row_stride = g.data_ptr(), stride
        dbranch = _lib.empty(tuple(g.shape), ctx.branch_dtype, g.device)
        P.dbranch, P.dbranch_row_stride = dbranch.data_ptr(), C
        _lib.launch("vivim_token_add_norm_bwd", P, g.device)
        return dres, dbranch, None, None


def _check_scale_tm(scale, res, rows):
    if scale is None:
        return
    if not (scale.dtype == torch.float32 and scale.dim() == 1 and scale.shape[0] == res.shape[0] and scale.is_contiguous()
            and scale.device == res.device and rows % scale.shape[0] == 0):
        raise ValueError("scale must be a contiguous (res.shape[0],) float32 tensor on res's device")


def _requires_grad(*ts):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def add_layer_norm_tm(res, branch, weight, bias, eps=1e-5, scale=None, out_dtype=None, rms=False, rows=None):
    """(res + scale * branch in res's dtype, the LayerNorm -- rms: RMSNorm -- of that sum as stored, in branch's dtype) for
    token-major rows.  `rows`: what tm_add_rows(res, branch, weight, bias) returned, from a caller that has just asked."""
    if out_dtype is not None and out_dtype != branch.dtype:
        raise ValueError(f"add_layer_norm_tm: a {branch.dtype} branch with a {out_dtype} output is not built")
    if not tm_add_pair_ok(branch.dtype, res.dtype):
        raise ValueError(f"add_layer_norm_tm: a {branch.dtype} branch on a {res.dtype} residual is not built")
    if rows is None:
        rows = tm_add_rows(res, branch, weight, bias)
        if rows is None or weight is None:
            raise ValueError("add_layer_norm_tm: unsupported tensors (tm_add_supported)")
    _check_scale_tm(scale, res, rows[0])
    return _AddNormTM.apply(res, branch, weight, bias, scale, eps, rms, _requires_grad(res, branch, weight, bias), rows, res.dtype)


def add_tm(res, branch, scale=None, rows=None):
    """res + scale * branch in res's dtype, contiguous, for token-major rows."""
    if not tm_add_pair_ok(branch.dtype, res.dtype):
        raise ValueError(f"add_tm: a {branch.dtype} branch on a {res.dtype} residual is not built")
    if rows is None:
        rows = tm_add_rows(res, branch)
        if rows is None:
            raise ValueError("add_tm: unsupported tensors (tm_add_supported)")
    _check_scale_tm(scale, res, rows[0])
    return _AddTM.apply(res, branch, scale, rows)


def norm_tm_no_residual(x, weight, bias, eps, rms, res_dtype=None):
    """(x in res_dtype or None, the norm of x in x's dtype): the first layer of a residual stream, which has nothing to add."""
    rows = tm_add_rows(x, x, weight, bias)
    if rows is None or weight is None:
        raise ValueError("norm_tm_no_residual: unsupported tensors (tm_add_supported)")
    if res_dtype is not None and not tm_add_pair_ok(x.dtype, res_dtype):
        raise ValueError(f"norm_tm_no_residual: {x.dtype} rows with a {res_dtype} residual are not built")
    return _AddNormTM.apply(None, x, weight, bias, None, eps, rms, _requires_grad(x, weight, bias), rows, res_dtype)


def rms_norm_tm(x, weight, bias=None, eps=1e-5, out_dtype=None):
    """RMSNorm of token-major rows: x * rsqrt(mean(x^2) + eps) * weight (+ bias), in x's dtype."""
    if out_dtype is not None and out_dtype != x.dtype:
        raise ValueError(f"rms_norm_tm: {x.dtype} rows with a {out_dtype} output are not built")
    return norm_tm_no_residual(x, weight, bias, eps, True)[1]
