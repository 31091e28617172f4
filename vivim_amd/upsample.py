"""Bilinear 2-D upsampling with a deterministic backward (csrc/upsample.hip; include/vivim_hip.h: vivim_upsample_params): the
decode head's `F.interpolate(x, size=size, mode="bilinear", align_corners=False)`.

    bilinear_upsample(x, size)   (N, C, H, W) -> (N, C, size[0], size[1]), fp32 / fp16 / bf16, differentiable; the output's
                                 memory format is the one ATen gives it (Tensor::suggest_memory_format)
    supported(x, size)           whether the kernels take this tensor as it lies in memory; where they do not (CPU tensors, other
                                 dtypes, downsampling on an axis) bilinear_upsample IS that F.interpolate call

Definition (ATen's), per axis in fp32: r = float(n_in) / float(n_out); src = max(0, r * (o + 0.5) - 0.5); i0 = int(src);
i1 = i0 + (i0 < n_in - 1); l1 = src - i0; l0 = 1 - l1.  The forward weighs four inputs, accumulates in fp32 and rounds once.
The backward is the transpose of that map in gather form: every dx element adds the dy elements whose taps name it, recomputed
with the forward's own expressions, in ascending output order.  No atomics, no workspace: the same kernels run whether or not
torch.use_deterministic_algorithms is on, and equal inputs give equal bits.  (ATen's backward scatters with float atomics -- in
the 16-bit type for fp16 / bf16 -- and raises under the strict flag.)

Two layouts: planes (contiguous NCHW: the logits and the edge map) and channels-last (dense NHWC memory: the decode-head
features, which SegformerMLP's (B, HW, C) output already is).  A tensor that is neither is made contiguous in its suggested
format first, as ATen does.  Equal input and output size launches nothing.  Under CUDA autocast upsample_bilinear2d is one of
the ops torch runs in fp32: so does this one (a 16-bit input is widened first, and the output is fp32, as ATen's is)."""
import os

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import ITYPE

_I31 = 2 ** 31 - 1


def _layout(x):
    """1 (channels-last) or 0 (planes): the memory format ATen gives the output, Tensor::suggest_memory_format() -- channels-last
    exactly when the strides are in channels-last order (c10's is_channels_last_strides_2d), contiguous otherwise."""
    sizes, strides = x.shape, x.stride()
    if strides[1] == 0:
        return 0
    least = 0
    for d in (1, 3, 2, 0):
        if sizes[d] == 0 or strides[d] < least or (d == 0 and least == strides[1]):
            return 0
        least = strides[d] * max(sizes[d], 1)
    return 1


def _format(layout):
    return torch.channels_last if layout == 1 else torch.contiguous_format


def _dense(x, layout):
    """Every image of x is dense in `layout`; the batch stride is free (sizes of 1 leave their stride free as well)."""
    N, C, H, W = x.shape
    want = (None, 1, W * C, C) if layout == 1 else (None, H * W, W, 1)
    return all(n == 1 or w is None or s == w for n, s, w in zip(x.shape, x.stride(), want)) and \
        (N == 1 or x.stride(0) >= C * H * W)


def _blocks(N, C, H, W, OH, OW, layout):
    """The larger of the two launches' workgroup counts (csrc/upsample.hip: upsample_blocks, element accesses)."""
    if layout == 1:
        return N * OH * -(-OW * C // 256)
    return N * C * max(-(-OH // 16) * -(-OW // 64), -(-H // 4) * -(-W // 64))


def supported(x, size):
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype in ITYPE and len(size) == 2):
        return False
    N, C, H, W = x.shape
    OH, OW = int(size[0]), int(size[1])
    if min(N, C, H, W) <= 0 or OH < H or OW < W:
        return False
    layout = _layout(x)
    if not _dense(x, layout):
        return False
    return (C * OH * OW <= _I31 and (2 * H + 3) * OH <= _I31 and (2 * W + 3) * OW <= _I31 and N * C <= _I31 and N * OH <= _I31
            and _blocks(N, C, H, W, OH, OW, layout) <= _I31)


def _empty(N, C, H, W, layout, like):
    if layout == 1:
        return _lib.empty((N, H, W, C), like.dtype, like.device).permute(0, 3, 1, 2)
    return _lib.empty((N, C, H, W), like.dtype, like.device)


def _params(shape, size, layout, dtype):
    P = _lib.UpsampleParams()
    P.batch, P.channels, P.in_h, P.in_w = shape
    P.out_h, P.out_w = size
    P.itype, P.layout = ITYPE[dtype], layout
    return P


class _BilinearUpsample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size):
        N, C, H, W = x.shape
        layout = _layout(x)
        ctx.shape, ctx.size, ctx.layout = (N, C, H, W), size, layout
        y = _empty(N, C, size[0], size[1], layout, x)
        if size == (H, W):
            return y.copy_(x)
        P = _params(ctx.shape, size, layout, x.dtype)
        P.x_batch_stride, P.y_batch_stride = x.stride(0), y.stride(0)
        P.x, P.y = x.data_ptr(), y.data_ptr()
        _lib.launch("vivim_upsample_bilinear2d_fwd", P, x.device)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        N, C, H, W = ctx.shape
        if ctx.size == (H, W):
            return dy, None
        if not _dense(dy, ctx.layout):
            dy = dy.contiguous(memory_format=_format(ctx.layout))
        dx = _empty(N, C, H, W, ctx.layout, dy)
        P = _params(ctx.shape, ctx.size, ctx.layout, dy.dtype)
        P.x_batch_stride, P.y_batch_stride = dx.stride(0), dy.stride(0)
        P.dy, P.dx = dy.data_ptr(), dx.data_ptr()
        _lib.launch("vivim_upsample_bilinear2d_bwd", P, dy.device)
        return dx, None


def bilinear_upsample(x, size):
    """F.interpolate(x, size=size, mode="bilinear", align_corners=False) through csrc/upsample.hip where `supported` says so
    (after making a tensor of neither layout contiguous in its suggested format), and that very call otherwise."""
    size = (int(size[0]), int(size[1]))
    if torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype in ITYPE and not os.environ.get("VIVIM_NO_UPSAMPLE"):
        if torch.is_autocast_enabled():                  # autocast's fp32 list holds upsample_bilinear2d: same dtypes as ATen
            x = x.float()
        if not _dense(x, _layout(x)):
            x = x.contiguous(memory_format=_format(_layout(x)))
        if supported(x, size):
            return _BilinearUpsample.apply(x, size)
    return F.interpolate(x, size=size, mode="bilinear", align_corners=False)
