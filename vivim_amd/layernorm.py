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
`add_norm_supported(x, branch, weight)` says whether they apply; the caller keeps its composition of torch ops otherwise."""
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


def layer_norm_cm(x, weight, bias, eps=1e-5):
    """F.layer_norm(x, (C,), weight, bias, eps) for a channel-major x; output dtype as ATen's under the ambient autocast state."""
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
