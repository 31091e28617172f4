"""The training decode head's upsample + dropout + concat as one op (csrc/head_concat.hip; include/vivim_hip_ext_head.h:
vivim_head_concat_params): what `Vivim.decode` does between the four projections and `linear_fuse`.

    upsample_concat(maps, size, p=None, keep=None)
                                 1 to 4 maps (N, C_s, H_s, W_s) in concat order, dense channels-last, one dtype out of fp32 / fp16 /
                                 bf16 -> (N, sum C_s, size[0], size[1]) with channels-last strides, in that dtype; differentiable
                                 in the maps.  p: None, or one dropout probability per map (None / 0: none for that map).  keep:
                                 None, or per map None or a uint8 mask (N, size[0], size[1], C_s), dense, 1 = keep; with p given
                                 and no mask, the masks are drawn by `draw_keep`.
    supported(maps, size, keep=None)
                                 whether the kernels take these tensors as they lie in memory; where they do not (CPU tensors,
                                 mixed dtypes, a map larger than the output, another layout, under autocast a dtype other than
                                 the autocast dtype) upsample_concat IS the stock composition: bilinear_upsample / F.interpolate
                                 per map, times mask and scale, torch.cat.
    draw_keep(shape, p, device)  the mask of one map: uint8, 1 with probability 1 - p, from torch's CUDA generator.

Definition, per element in fp32: v is the bilinear value of upsample.py (the same taps, the same expression order), and
y = round(keep ? v * scale_s : 0) with scale_s = float32(1 / (1 - p_s)), 1 without dropout.  A map of the output's own size is
y = round(keep ? x * scale_s : 0).  One rounding per output: under bf16 autocast the stock route upsamples into fp32, drops out
in fp32 and rounds once at linear_fuse's cast -- the same single rounding, without the fp32 tensors.  The backward is the transpose
in gather form (upsample.py): a dx element adds weight * (keep ? dy * scale_s : 0) over its window in ascending order in fp32 and
is rounded once.  No atomics, no workspace; the same kernels run whether or not torch.use_deterministic_algorithms is on, and
equal inputs and masks give equal bits.  One launch forward, one backward, whatever the number of maps.

The masks come from the distribution of F.dropout's (independent Bernoulli(1 - p) per element) but not from its bits: a run with
this op does not reproduce the stock route's random stream on the device -- as with vivim.DropPath against SegformerDropPath."""
import ctypes

import torch

from . import _lib
from . import upsample as _up
from ._lib import ITYPE

_I31 = 2 ** 31 - 1


def draw_keep(shape, p, device):
    """uint8 `shape`, 1 with probability 1 - p: torch's CUDA generator (one rand + one compare)."""
    return (torch.rand(shape, device=device) >= p).to(torch.uint8)


def _scale(p):
    """float32(1 / (1 - p)) as a Python float: what the kernels multiply by."""
    return float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))


def _probs(p, n):
    p = [None] * n if p is None else [None if q is None or float(q) == 0.0 else float(q) for q in p]
    if len(p) != n or any(q is not None and not 0.0 < q < 1.0 for q in p):
        raise ValueError(f"upsample_concat: p = {p}: one probability in [0, 1) per map")
    return p


def _dense_cl(x):
    """Every image of x is dense channels-last memory; the batch stride is free (sizes of 1 leave their stride free as well)."""
    return _up._dense(x, 1)


def _batch_stride(x):
    """x.stride(0), or the size of the one image where that stride is free."""
    return x.stride(0) if x.shape[0] > 1 else x[0].numel()


def supported(maps, size, keep=None):
    if not (isinstance(maps, (list, tuple)) and 1 <= len(maps) <= 4 and len(size) == 2):
        return False
    if not all(torch.is_tensor(x) and x.is_cuda and x.dim() == 4 for x in maps):
        return False
    x0 = maps[0]
    if x0.dtype not in ITYPE or any(x.dtype != x0.dtype or x.device != x0.device or x.shape[0] != x0.shape[0] for x in maps):
        return False
    if torch.is_autocast_enabled() and x0.dtype != torch.get_autocast_dtype("cuda"):
        return False                                     # the stock route's dtypes under autocast are not this op's
    OH, OW = int(size[0]), int(size[1])
    N, total = x0.shape[0], sum(x.shape[1] for x in maps)
    if N <= 0 or total * OH * OW > _I31 - 256 or N * OH > _I31:
        return False
    blocks = 0
    for s, x in enumerate(maps):
        _, C, H, W = x.shape
        if min(C, H, W) <= 0 or H > OH or W > OW or not _dense_cl(x):
            return False
        if (2 * H + 3) * OH > _I31 or (2 * W + 3) * OW > _I31:
            return False
        blocks += N * OH * -(-OW * C // 256)             # the forward's grid with element accesses: the larger of the two
        k = None if keep is None else keep[s]
        if k is not None and not (torch.is_tensor(k) and k.dtype == torch.uint8 and k.device == x.device
                                  and tuple(k.shape) == (N, OH, OW, C) and k.is_contiguous()):
            return False
    return blocks <= _I31


def _params(shapes, size, dtype, scales, keep):
    P = _lib.HeadConcatParams()
    P.struct_bytes = ctypes.sizeof(P)
    P.batch, P.n_maps, P.itype = shapes[0][0], len(shapes), ITYPE[dtype]
    P.out_h, P.out_w = size
    off = 0
    for s, (_, C, H, W) in enumerate(shapes):
        P.map_c[s], P.map_h[s], P.map_w[s], P.chan_off[s], P.scale[s] = C, H, W, off, scales[s]
        if keep[s] is not None:
            P.keep[s], P.keep_batch_stride[s] = keep[s].data_ptr(), _batch_stride(keep[s])
        off += C
    P.out_pixel_stride = off
    return P


class _UpsampleConcat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, size, scales, keep, *maps):
        shapes = [tuple(x.shape) for x in maps]
        N, total = shapes[0][0], sum(sh[1] for sh in shapes)
        out = _lib.empty((N, size[0], size[1], total), maps[0].dtype, maps[0].device).permute(0, 3, 1, 2)
        P = _params(shapes, size, maps[0].dtype, scales, keep)
        P.out, P.out_batch_stride = out.data_ptr(), _batch_stride(out)
        for s, x in enumerate(maps):
            P.maps[s], P.map_batch_stride[s] = x.data_ptr(), _batch_stride(x)
        _lib.launch("vivim_head_concat_fwd", P, out.device)
        ctx.shapes, ctx.size, ctx.scales, ctx.keep = shapes, size, scales, keep
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        if not _dense_cl(dy):
            dy = dy.contiguous(memory_format=torch.channels_last)
        P = _params(ctx.shapes, ctx.size, dy.dtype, ctx.scales, ctx.keep)
        P.dout, P.out_batch_stride = dy.data_ptr(), _batch_stride(dy)
        dmaps = []
        for s, (N, C, H, W) in enumerate(ctx.shapes):
            dx = _lib.empty((N, H, W, C), dy.dtype, dy.device).permute(0, 3, 1, 2)
            P.dmaps[s], P.dmap_batch_stride[s] = dx.data_ptr(), _batch_stride(dx)
            dmaps.append(dx)
        _lib.launch("vivim_head_concat_bwd", P, dy.device)
        return (None, None, None) + tuple(dmaps)


def _stock(maps, size, p, keep):
    """The stock composition: upsample each map, multiply by mask and scale, concatenate."""
    feats = []
    for s, x in enumerate(maps):
        y = _up.bilinear_upsample(x, size)
        if p[s] is not None or (keep is not None and keep[s] is not None):
            k = keep[s] if keep is not None and keep[s] is not None else draw_keep((x.shape[0], size[0], size[1], x.shape[1]), p[s], x.device)
            scale = _scale(p[s]) if p[s] is not None else 1.0
            y = y * (k.permute(0, 3, 1, 2).to(y.dtype) * scale)
        feats.append(y)
    return torch.cat(feats, dim=1)


def upsample_concat(maps, size, p=None, keep=None):
    """The maps upsampled to `size`, dropped out per element and concatenated along the channels, through csrc/head_concat.hip
    where `supported` says so and as the stock composition otherwise."""
    maps, size = list(maps), (int(size[0]), int(size[1]))
    p = _probs(p, len(maps))
    if keep is not None and len(keep) != len(maps):
        raise ValueError(f"upsample_concat: {len(keep)} masks for {len(maps)} maps")
    if not supported(maps, size, keep):
        return _stock(maps, size, p, keep)
    keep = [None] * len(maps) if keep is None else list(keep)
    for s, x in enumerate(maps):
        if keep[s] is None and p[s] is not None:
            keep[s] = draw_keep((x.shape[0], size[0], size[1], x.shape[1]), p[s], x.device)
    scales = [1.0 if q is None else _scale(q) for q in p]
    return _UpsampleConcat.apply(size, scales, keep, *maps)
