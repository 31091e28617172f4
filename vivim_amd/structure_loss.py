"""The structure loss: boundary-weighted BCE + weighted IoU with the weight map 1 + 5 * |avgpool31(mask) - mask| -- the criterion of
the reference's binary and polyp recipes (complements/train_binary.py:57-67, modeling/utils.py:89-100) and its
`multiclass_structure_loss` (final_multiclass_training.py:403-445) -- as an eager composition and as three launches
(csrc/structure_loss.hip; include/vivim_hip_ext.h: vivim_structure_loss_params).

    multiclass_structure_loss(logits, targets, num_classes, eps=1e-6)   eager; logits (N, C, H, W), targets (N, H, W) integer labels
    structure_loss(pred, mask, eps=1.0)                                  eager; pred and mask (N, 1, H, W), mask of zeros and ones
    multiclass_structure_loss_fused(...), structure_loss_fused(...)      the same through the kernels where `supported` says so,
                                                                         the eager function unchanged otherwise
    supported(logits, targets, num_classes, first_class=0)               CUDA tensors, logits fp32 / fp16 / bf16 with contiguous
                                                                         planes (batch and channel strides free), targets int64
                                                                         or uint8 (N, H, W) with contiguous rows, 1 to 8 classes

Per (image, channel), with m the mask, k the number of mask pixels in the 31 x 31 window clipped to the image and w = 1 + 5 * |k / 961 - m|:
loss_nc = sum(w * bce) / sum(w) + 1 - (sum(w * s * m) + eps) / (sum(w * (s + m - s * m)) + eps), loss = mean over (n, c).  A label
that matches no channel is a pixel of no class (labels are only compared), as in seg_loss and seg_metrics.

Two departures from the reference's text, both on purpose.  The masks come from comparisons instead of F.one_hot, which raises on a
label >= C.  And the binary recipes spell the BCE's keyword `reduce='none'`, which torch reads as the legacy flag reduce=True, so what
they run is the UNWEIGHTED mean BCE plus the weighted IoU; `structure_loss` here is the boundary-weighted form the multiclass function
has (reduction='none'), i.e. the multiclass formula with one channel, label 1 and eps = 1.

The kernels keep nothing per pixel for autograd (the logits, the targets and 3 * N * C floats, against about ten (N, C, H, W) fp32
tensors of the eager chain), form neither 1 - sigmoid nor union - inter by subtraction, and use no atomics: loss and gradient are
bit-repeatable.  The upstream gradient is read on the device and multiplied in fp32 before dlogits is rounded to the logits' dtype."""
import ctypes

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import ITYPE

_TTYPE = {torch.int64: 0, torch.uint8: 1}
MAX_CLASSES = 8


def _structure_terms(x, mask, eps):
    """(N, C) per-image, per-channel loss from logits x and a 0 / 1 mask of the same shape and dtype."""
    weit = 1 + 5 * torch.abs(F.avg_pool2d(mask, kernel_size=31, stride=1, padding=15) - mask)
    wbce = F.binary_cross_entropy_with_logits(x, mask, reduction="none")
    wbce = (weit * wbce).sum(dim=(2, 3)) / weit.sum(dim=(2, 3))
    prob = torch.sigmoid(x)
    inter = (prob * mask * weit).sum(dim=(2, 3))
    union = ((prob + mask) * weit).sum(dim=(2, 3))
    return wbce + 1 - (inter + eps) / (union - inter + eps)


def _widen(x):
    return x.float() if x.dtype in (torch.float16, torch.bfloat16) else x


def multiclass_structure_loss(logits, targets, num_classes, eps=1e-6):
    """final_multiclass_training.py:403-445, all channels at once: logits (N, C, H, W), targets (N, H, W) -> 0-dim loss."""
    x = _widen(logits)
    classes = torch.arange(num_classes, device=targets.device)[None, :, None, None]
    mask = (targets.long()[:, None] == classes).to(x.dtype)
    return _structure_terms(x, mask, eps).mean()


def structure_loss(pred, mask, eps=1.0):
    """The binary form (train_binary.py:57-67 with the BCE weighted as intended, see above): pred, mask (N, 1, H, W) -> 0-dim loss."""
    x = _widen(pred)
    return _structure_terms(x, mask.to(x.dtype), eps).mean()


def supported(logits, targets, num_classes, first_class=0):
    if not (torch.is_tensor(logits) and torch.is_tensor(targets) and logits.is_cuda and targets.is_cuda
            and logits.device == targets.device):
        return False
    if not (logits.dim() == 4 and logits.dtype in ITYPE and targets.dim() == 3 and targets.dtype in _TTYPE):
        return False
    N, C, H, W = logits.shape
    if not (C == num_classes and 1 <= C <= MAX_CLASSES and 0 <= first_class <= 255 and N > 0 and 0 < H * W < 2 ** 31 - 4096
            and N * (H // 16 + 1) * (W // 64 + 1) < 2 ** 31):
        return False
    if tuple(targets.shape) != (N, H, W):
        return False
    return (logits.stride(3) == 1 and logits.stride(2) == W and targets.stride(2) == 1 and targets.stride(1) == W)


def _params(logits, targets, first_class, eps):
    N, C, H, W = logits.shape
    P = _lib.StructureLossParams()
    P.struct_bytes = ctypes.sizeof(P)
    P.batch, P.classes, P.height, P.width = N, C, H, W
    P.itype, P.ttype, P.first_class, P.eps = ITYPE[logits.dtype], _TTYPE[targets.dtype], first_class, eps
    P.logits_batch_stride, P.logits_c_stride, P.target_batch_stride = logits.stride(0), logits.stride(1), targets.stride(0)
    P.logits, P.target = logits.data_ptr(), targets.data_ptr()
    return P


class _StructureLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, first_class, eps, track):
        N, C = logits.shape[:2]
        P = _params(logits, targets, first_class, eps)
        ws_bytes = _lib.lib().vivim_structure_loss_workspace_bytes(P)
        # one buffer: the partial-sum slots, then (only when a backward can follow) the (N, C, 3) factors of the gradient
        buf = _lib.empty((ws_bytes // 4 + (3 * N * C if track else 0),), torch.float32, logits.device)
        loss = _lib.empty((), torch.float32, logits.device)
        P.workspace, P.workspace_bytes, P.loss = buf.data_ptr(), ws_bytes, loss.data_ptr()
        P.coef = buf.data_ptr() + ws_bytes if track else None
        _lib.launch("vivim_structure_loss_fwd", P, logits.device)
        if track:
            ctx.save_for_backward(logits, targets, buf[ws_bytes // 4:])
            ctx.first_class, ctx.eps = first_class, eps
        else:
            ctx.mark_non_differentiable(loss)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        logits, targets, coef = ctx.saved_tensors
        N, C, H, W = logits.shape
        go = grad_out
        if go.dtype != torch.float32 or go.device != logits.device:
            go = go.to(device=logits.device, dtype=torch.float32)
        go = go.contiguous()                                                 # a 0-dim tensor: the kernel reads *grad_out itself
        dlogits = _lib.empty((N, C, H, W), logits.dtype, logits.device)
        P = _params(logits, targets, ctx.first_class, ctx.eps)
        P.coef, P.grad_out, P.dlogits = coef.data_ptr(), go.data_ptr(), dlogits.data_ptr()
        P.dlogits_batch_stride, P.dlogits_c_stride = C * H * W, H * W
        _lib.launch("vivim_structure_loss_bwd", P, logits.device)
        return dlogits, None, None, None, None


def _fused(logits, targets, first_class, eps):
    track = torch.is_grad_enabled() and logits.requires_grad
    return _StructureLoss.apply(logits, targets, int(first_class), float(eps), track)


def multiclass_structure_loss_fused(logits, targets, num_classes, eps=1e-6):
    """multiclass_structure_loss(logits, targets, num_classes, eps) through the fused kernels where `supported` says so, that
    function itself otherwise."""
    if not supported(logits, targets, num_classes):
        return multiclass_structure_loss(logits, targets, num_classes, eps)
    return _fused(logits, targets, 0, eps)


def _binary_labels(pred, mask):
    """The (N, H, W) uint8 label map of a (N, 1, H, W) mask of zeros and ones, or None where the kernels do not apply.  A bool mask is
    taken as it is; any other dtype is checked to hold nothing but 0 and 1, which is one host synchronisation."""
    if not (torch.is_tensor(pred) and torch.is_tensor(mask) and pred.is_cuda and mask.is_cuda and pred.dim() == 4 and mask.dim() == 4
            and pred.shape[1] == 1 and mask.shape == pred.shape):
        return None
    if mask.dtype != torch.bool and not bool(((mask == 0) | (mask == 1)).all()):
        return None
    return mask.to(torch.uint8).reshape(mask.shape[0], mask.shape[2], mask.shape[3]).contiguous()


def structure_loss_fused(pred, mask, eps=1.0):
    """structure_loss(pred, mask, eps) through the fused kernels (one channel whose label is 1) where they apply -- CUDA tensors, a
    supported layout, a mask that is exactly {0, 1} -- and that function itself otherwise."""
    labels = _binary_labels(pred, mask)
    if labels is None or not supported(pred, labels, 1, 1):
        return structure_loss(pred, mask, eps)
    return _fused(pred, labels, 1, eps)
