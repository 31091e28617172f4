"""The train step's loss as three launches (csrc/seg_loss.hip; include/vivim_hip.h: vivim_seg_loss_params): 0.4 * class-balanced
focal + 0.6 * Tversky over softmax(logits), the formulas of train_step.recall_focused_loss.

    recall_focused_loss_fused(logits, targets, num_classes, gamma=2.0, alpha=None) -> 0-dim f32 loss
                                            logits (N, C, H, W) fp32 / fp16 / bf16, pixels contiguous (batch and channel strides
                                            free: a channel slice of a wider tensor is taken as it is); targets (N, H, W) int64
                                            or uint8; a label outside [0, C) is a pixel of no class (labels are only compared)
    supported(logits, targets, num_classes, gamma)   whether the kernels take these tensors; where they do not (CPU tensors, other
                                            layouts, gamma != 2, more than 8 classes) the function returns
                                            train_step.recall_focused_loss(...) unchanged

Forward: partial sums per (image, workgroup) + one finalise kernel; backward: one kernel that recomputes the softmax.  What
autograd keeps is the logits, the targets and 2 * N * C floats, against about ten (N, C, H, W) fp32 tensors of the eager chain.
1 - p is never formed by subtraction, so the fp32 gradient holds to ~5e-7 of an fp64 evaluation at any logit scale (the eager
composition loses three digits and more once the softmax is confident).  No float atomics: loss and gradient are bit-repeatable.
The upstream gradient is read on the device and multiplied in fp32 before dlogits is rounded to the logits' dtype."""
import torch

from . import _lib
from ._lib import ITYPE
from .train_step import _alpha_tensor, recall_focused_loss

_TTYPE = {torch.int64: 0, torch.uint8: 1}
FOCAL_WEIGHT, TVERSKY_WEIGHT, TVERSKY_ALPHA, TVERSKY_BETA, SMOOTH, EPS = 0.4, 0.6, 0.3, 0.7, 1e-6, 1e-6


def supported(logits, targets, num_classes, gamma=2.0):
    if not (torch.is_tensor(logits) and torch.is_tensor(targets) and logits.is_cuda and targets.is_cuda
            and logits.device == targets.device):
        return False
    if not (logits.dim() == 4 and logits.dtype in ITYPE and targets.dim() == 3 and targets.dtype in _TTYPE):
        return False
    N, C, H, W = logits.shape
    if not (C == num_classes and 2 <= C <= 8 and gamma == 2 and N > 0 and 0 < H * W < 2 ** 31 and N * 64 < 2 ** 31):
        return False
    if tuple(targets.shape) != (N, H, W):
        return False
    return (logits.stride(3) == 1 and logits.stride(2) == W and targets.stride(2) == 1 and targets.stride(1) == W)


def _params(logits, targets, alpha):
    N, C, H, W = logits.shape
    P = _lib.SegLossParams()
    P.batch, P.classes, P.pixels, P.itype, P.ttype = N, C, H * W, ITYPE[logits.dtype], _TTYPE[targets.dtype]
    P.gamma, P.focal_weight, P.tversky_weight = 2.0, FOCAL_WEIGHT, TVERSKY_WEIGHT
    P.tversky_alpha, P.tversky_beta, P.smooth, P.eps = TVERSKY_ALPHA, TVERSKY_BETA, SMOOTH, EPS
    P.logits_batch_stride, P.logits_c_stride, P.target_batch_stride = logits.stride(0), logits.stride(1), targets.stride(0)
    P.logits, P.target, P.alpha = logits.data_ptr(), targets.data_ptr(), alpha.data_ptr()
    return P


class _RecallFocusedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, alpha, track):
        N, C = logits.shape[:2]
        P = _params(logits, targets, alpha)
        ws_bytes = _lib.lib().vivim_seg_loss_workspace_bytes(P)
        # one buffer: the partial-sum slots, then (only when a backward can follow) the (N, C, 2) Tversky gradient factors
        buf = _lib.empty((ws_bytes // 4 + (2 * N * C if track else 0),), torch.float32, logits.device)
        loss = _lib.empty((), torch.float32, logits.device)
        P.workspace, P.workspace_bytes, P.loss = buf.data_ptr(), ws_bytes, loss.data_ptr()
        P.coef = buf.data_ptr() + ws_bytes if track else None
        _lib.launch("vivim_seg_loss_fwd", P, logits.device)
        if track:
            ctx.save_for_backward(logits, targets, alpha, buf)
            ctx.ws_bytes = ws_bytes
        else:
            ctx.mark_non_differentiable(loss)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        logits, targets, alpha, buf = ctx.saved_tensors
        N, C, H, W = logits.shape
        go = grad_out
        if go.dtype != torch.float32 or go.device != logits.device:
            go = go.to(device=logits.device, dtype=torch.float32)
        go = go.contiguous()                                                 # a 0-dim tensor: the kernel reads *grad_out itself
        dlogits = _lib.empty((N, C, H, W), logits.dtype, logits.device)
        P = _params(logits, targets, alpha)
        P.coef, P.grad_out, P.dlogits = buf.data_ptr() + ctx.ws_bytes, go.data_ptr(), dlogits.data_ptr()
        P.dlogits_batch_stride, P.dlogits_c_stride = C * H * W, H * W
        _lib.launch("vivim_seg_loss_bwd", P, logits.device)
        return dlogits, None, None, None


def recall_focused_loss_fused(logits, targets, num_classes, gamma=2.0, alpha=None):
    """train_step.recall_focused_loss(logits, targets, num_classes, gamma, alpha=alpha) through the fused kernels where
    `supported` says so, that function itself otherwise.  `alpha`: None (its defaults), a tuple, or an f32 device tensor (C,)."""
    if not supported(logits, targets, num_classes, gamma):
        return recall_focused_loss(logits, targets, num_classes, gamma, alpha=alpha)
    if alpha is None:
        alpha = (0.05, 0.475, 0.475) if num_classes == 3 else tuple([1.0 / num_classes] * num_classes)
    if torch.is_tensor(alpha):
        a = alpha.detach().to(device=logits.device, dtype=torch.float32).contiguous()
    else:
        a = _alpha_tensor(alpha, logits.device, torch.float32)              # built once: no host-to-device copy per step
    if a.numel() != num_classes:
        return recall_focused_loss(logits, targets, num_classes, gamma, alpha=alpha)
    track = torch.is_grad_enabled() and logits.requires_grad
    return _RecallFocusedLoss.apply(logits, targets, a, track)
