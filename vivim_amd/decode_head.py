"""The decode head of an eval-mode, no-grad forward as four folded projections and one kernel (csrc/decode_head.hip;
include/vivim_hip.h: vivim_decode_head_params).

In eval mode everything the stock head does before its ReLU is linear: BatchNorm is a per-channel affine map of its running
statistics, the dropouts are identities, and bilinear upsampling commutes with a 1x1 convolution.  So linear_fuse, BatchNorm
and the four per-stage projections fold into four matrices W'_s (hidden x C_s) and one bias vector, and with m_s = W'_s x_s at
stage s's own resolution the head is

    logits = W_out . relu(sum_s up(m_s) + bias) + b_out

    fold_decode_head(decoder, out_conv)             -> ([W'_0 .. W'_3], bias, w_out, b_out): fp64 arithmetic, rounded once to fp32
    fused_decode_head(maps, bias, w_out, b_out, size)   the kernel: maps[s] is (N, H_s, W_s, hidden) channels-last memory (what
                                                    F.linear leaves for token-major input), -> (N, classes, size[0], size[1])
    supported(maps, bias, w_out, b_out, size)       whether the kernel takes these tensors as they lie in memory
    applies(vivim, states) / eval_decode(vivim, states)   the gate and the whole head, as Vivim.decode uses them

There is no backward and no training-mode form (the per-map dropout sits after the upsampling and does not commute)."""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import ITYPE

_I31 = 2 ** 31 - 1
MAX_HIDDEN = 1024          # csrc/decode_head.hip: bias and w_out live in LDS
MAX_CLASSES = 8
MAX_MAPS = 4
_TILE = 8


def _projections(decoder):
    """The per-stage nn.Linear layers of either transformers layout."""
    mlps = decoder.linear_c if hasattr(decoder, "linear_c") else decoder.linear_projections
    return [m.proj for m in mlps]


def fold_decode_head(decoder, out_conv):
    """-> (weights, bias, w_out, b_out) of the folded eval-mode head: weights[s] (hidden, C_s), bias (hidden,), w_out
    (classes, hidden), b_out (classes,) or None, all fp32 on the parameters' device, computed in fp64 and rounded once.
    The concat is feats[::-1]: stage s meets columns [(n - 1 - s) * hidden, (n - s) * hidden) of linear_fuse.weight."""
    projs = _projections(decoder)
    bn, fuse = decoder.batch_norm, decoder.linear_fuse
    n, hidden = len(projs), fuse.out_channels
    with torch.no_grad():
        wf = fuse.weight.double().reshape(hidden, -1)
        a = torch.rsqrt(bn.running_var.double() + bn.eps)
        if bn.weight is not None:
            a = a * bn.weight.double()
        bias = -a * bn.running_mean.double()
        if bn.bias is not None:
            bias = bias + bn.bias.double()
        if fuse.bias is not None:
            bias = bias + a * fuse.bias.double()
        weights = []
        for s, proj in enumerate(projs):
            blk = wf[:, (n - 1 - s) * hidden:(n - s) * hidden]
            weights.append((a[:, None] * (blk @ proj.weight.double())).float().contiguous())
            if proj.bias is not None:
                bias = bias + a * (blk @ proj.bias.double())
        w_out = out_conv.weight.double().reshape(out_conv.out_channels, -1).float().contiguous()
        b_out = None if out_conv.bias is None else out_conv.bias.detach().float().contiguous()
    return weights, bias.float().contiguous(), w_out, b_out


def _image_dense(m):
    """(N, H, W, K) with every image dense; the batch stride is free but no smaller than an image."""
    N, H, W, K = m.shape
    want = (None, W * K, K, 1)
    return all(n == 1 or w is None or s == w for n, s, w in zip(m.shape, m.stride(), want)) and (N == 1 or m.stride(0) >= H * W * K)


def supported(maps, bias, w_out, b_out, size):
    if not (1 <= len(maps) <= MAX_MAPS and len(size) == 2 and all(torch.is_tensor(m) and m.dim() == 4 for m in maps)):
        return False
    m0 = maps[0]
    if not (m0.is_cuda and m0.dtype in ITYPE):
        return False
    N, _, _, K = m0.shape
    OH, OW = int(size[0]), int(size[1])
    small = [bias, w_out] + ([] if b_out is None else [b_out])
    if not all(torch.is_tensor(t) and t.device == m0.device and t.dtype == torch.float32 and t.is_contiguous() for t in small):
        return False
    if w_out.dim() != 2 or not 1 <= w_out.shape[0] <= MAX_CLASSES or not 1 <= K <= MAX_HIDDEN:
        return False
    C = w_out.shape[0]
    if w_out.shape[1] != K or tuple(bias.shape) != (K,) or (b_out is not None and tuple(b_out.shape) != (C,)):
        return False
    for m in maps:
        if m.device != m0.device or m.dtype != m0.dtype or m.shape[0] != N or m.shape[3] != K or not _image_dense(m):
            return False
        H, W = m.shape[1], m.shape[2]
        if min(N, H, W) <= 0 or H > OH or W > OW or K * H * W > _I31:
            return False
    return C * OH * OW <= _I31 and N * -(-OH // _TILE) * -(-OW // _TILE) <= _I31


def _params(maps, bias, w_out, b_out, logits, size):
    P = _lib.DecodeHeadParams()
    P.struct_bytes = ctypes.sizeof(_lib.DecodeHeadParams)
    P.batch, P.hidden, P.classes, P.n_maps = maps[0].shape[0], maps[0].shape[3], w_out.shape[0], len(maps)
    P.out_h, P.out_w = size
    P.itype = ITYPE[maps[0].dtype]
    for s, m in enumerate(maps):
        P.map_h[s], P.map_w[s] = m.shape[1], m.shape[2]
        P.map_batch_stride[s] = max(m.stride(0), m.shape[1] * m.shape[2] * m.shape[3])      # N == 1 leaves the stride free
        P.maps[s] = m.data_ptr()
    P.logits_batch_stride = max(logits.stride(0), logits.shape[1] * logits.shape[2] * logits.shape[3])
    P.bias, P.w_out, P.b_out, P.logits = bias.data_ptr(), w_out.data_ptr(), _lib.ptr(b_out), logits.data_ptr()
    return P


def fused_decode_head(maps, bias, w_out, b_out, size, out=None):
    """logits (N, classes, size[0], size[1]) in the maps' dtype: relu(sum_s upsample(maps[s]) + bias) contracted with w_out, plus
    b_out (None: no bias).  maps[s] is (N, H_s, W_s, hidden), each image dense, H_s <= size[0], W_s <= size[1]; bias, w_out and
    b_out are contiguous fp32.  `out`, if given, receives the logits: every image contiguous planes, the batch stride free.
    No fallback: tensors the kernel does not take (`supported`) raise."""
    maps, size = list(maps), (int(size[0]), int(size[1]))
    _lib.check(supported(maps, bias, w_out, b_out, size), "fused_decode_head: unsupported tensors (decode_head.supported)")
    N, C = maps[0].shape[0], w_out.shape[0]
    if out is None:
        out = _lib.empty((N, C, size[0], size[1]), maps[0].dtype, maps[0].device)
    else:
        _lib.check(out.shape == (N, C, size[0], size[1]) and out.dtype == maps[0].dtype and out.device == maps[0].device
                   and out[0].is_contiguous() and (N == 1 or out.stride(0) >= C * size[0] * size[1]),
                   "fused_decode_head: out must be (N, classes, H, W) planes of the maps' dtype")
    _lib.launch("vivim_decode_head_fwd", _params(maps, bias, w_out, b_out, out, size), maps[0].device)
    return out


# ---- the head inside Vivim ------------------------------------------------------------------------------------------------------
def _is_1x1(conv):
    return (isinstance(conv, nn.Conv2d) and conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.groups == 1
            and conv.padding == (0, 0))


def _fold_inputs(vivim):
    """Every tensor the fold reads."""
    dec, bn = vivim.decoder, vivim.decoder.batch_norm
    ts = []
    for proj in _projections(dec):
        ts += [proj.weight, proj.bias]
    ts += [dec.linear_fuse.weight, dec.linear_fuse.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var,
           vivim.out.weight, vivim.out.bias]
    return [t for t in ts if t is not None]


def _folded(vivim):
    """The fold of vivim's head, cached on the module and rebuilt when any tensor that enters it was written in place or
    replaced (load_state_dict, an optimizer step, .to()): {"key", "bias", "w_out", "b_out", "weights": {dtype: [W'_s]}}."""
    key = tuple((t._version, t.data_ptr()) for t in _fold_inputs(vivim))
    cache = vivim.__dict__.get("_decode_head_fold")
    if cache is None or cache["key"] != key:
        weights, bias, w_out, b_out = fold_decode_head(vivim.decoder, vivim.out)
        cache = {"key": key, "bias": bias, "w_out": w_out, "b_out": b_out, "weights": {torch.float32: weights}, "format": {}}
        vivim.__dict__["_decode_head_fold"] = cache
    return cache


def _compute_dtype(states):
    if torch.is_autocast_enabled():
        return torch.get_autocast_dtype("cuda")
    return states[0].dtype


def applies(vivim, states):
    """Whether Vivim.decode may take eval_decode for these encoder states: eval mode and no grad (there is no backward), CUDA
    tensors of a kernel dtype, a head of the stock form (1x1 linear_fuse and out, BatchNorm with running statistics, ReLU) and
    shapes the kernel takes."""
    dec = vivim.decoder
    if vivim.training or torch.is_grad_enabled():
        return False
    if not (1 <= len(states) <= MAX_MAPS and all(torch.is_tensor(x) and x.is_cuda and x.dim() == 4 for x in states)):
        return False
    bn = dec.batch_norm
    if not (isinstance(bn, nn.BatchNorm2d) and bn.track_running_stats and bn.running_mean is not None
            and type(dec.activation) is nn.ReLU and _is_1x1(dec.linear_fuse) and _is_1x1(vivim.out)):
        return False
    projs = _projections(dec)
    hidden, classes = dec.linear_fuse.out_channels, vivim.out.out_channels
    if not (len(projs) == len(states) and dec.linear_fuse.in_channels == hidden * len(projs) and vivim.out.in_channels == hidden
            and all(p.out_features == hidden and p.in_features == x.shape[1] for p, x in zip(projs, states))):
        return False
    if _compute_dtype(states) not in ITYPE or any(x.dtype not in ITYPE or x.device != states[0].device for x in states):
        return False
    if not torch.is_autocast_enabled() and any(x.dtype != p.weight.dtype for p, x in zip(projs, states)):
        return False                                     # the stock path's own error
    if vivim.out.weight.device != states[0].device or not 1 <= hidden <= MAX_HIDDEN or not 1 <= classes <= MAX_CLASSES:
        return False
    N, _, OH, OW = states[0].shape
    if any(x.shape[0] != N or min(x.shape) <= 0 or x.shape[2] > OH or x.shape[3] > OW or hidden * x.shape[2] * x.shape[3] > _I31
           for x in states):
        return False
    return classes * OH * OW <= _I31 and N * -(-OH // _TILE) * -(-OW // _TILE) <= _I31


def _stock_channels_last(vivim, cache, dtype, device):
    """Whether the stock head's logits come out in channels-last memory here: its 1x1 convolutions see channels-last input (the
    projected maps are (N, HW, C) memory), and what the convolution backend returns for that differs between builds.  Asked
    once per fold and dtype, of `out` itself on a 2 x 2 input."""
    fmt = cache["format"].get(dtype)
    if fmt is None:
        probe = torch.zeros(1, 2, 2, vivim.out.in_channels, dtype=dtype, device=device).permute(0, 3, 1, 2)
        y = vivim.out(probe)
        fmt = cache["format"][dtype] = bool(y.is_contiguous(memory_format=torch.channels_last) and not y.is_contiguous())
    return fmt


def eval_decode(vivim, states):
    """The eval-mode head of `vivim` on the encoder states (N, C_s, H_s, W_s): per stage one F.linear with the folded weight on
    the view SegformerMLP itself makes (token-major (N, HW, hidden) out: the kernel's layout), then the kernel.  Under autocast
    the projections run, and the logits come out, in the autocast dtype, as the stock `out` convolution's do."""
    cache = _folded(vivim)
    dtype = _compute_dtype(states)
    weights = cache["weights"].get(dtype)
    if weights is None:                                  # one copy per compute dtype: a call adds no cast launches
        weights = cache["weights"][dtype] = [w.to(dtype) for w in cache["weights"][torch.float32]]
    maps = []
    for x, w in zip(states, weights):
        N, _, H, W = x.shape
        maps.append(F.linear(x.flatten(2).transpose(1, 2), w).view(N, H, W, -1))
    size = tuple(states[0].shape[2:])
    logits = fused_decode_head(maps, cache["bias"], cache["w_out"], cache["b_out"], size)
    if _stock_channels_last(vivim, cache, dtype, logits.device):
        logits = logits.contiguous(memory_format=torch.channels_last)
    return logits
