"""Validation metrics on the device (csrc/seg_metrics.hip; include/vivim_hip.h: vivim_seg_metrics_params): what the reference's
validation loop does with every batch of logits after the loss -- argmax, then MulticlassMetricsTracker -- without moving the
logits to the host.

    seg_confusion_counts(logits, targets, num_classes, return_preds=False) -> int32 (N, C, 3) = {tp, fp, fn} per (image, class)
                                            [, uint8 (N, H, W) prediction map]
                                            logits (N, C, H, W) fp32 / fp16 / bf16, pixels contiguous (batch and channel strides
                                            free); targets (N, H, W) int64 or uint8
    supported(logits, targets, num_classes) whether the kernels take these tensors; where they do not (CPU tensors, other layouts,
                                            more than 8 classes) the same definition runs as an eager torch composition
    SegMetricsTracker(num_classes=3)        reset() / update(logits, targets) / get_results(): the reference tracker's surface;
                                            update() launches two kernels and neither synchronises nor copies anything to the
                                            host, get_results() copies the (C, 7) fp64 `state` once

Semantics.  The prediction of a pixel is the FIRST index of the maximum of its C logits, compared in their own values (no
softmax); a NaN counts as the maximum and the first NaN wins (numpy.argmax's rule).  Labels are only compared with the class
index: a label outside [0, C) is a pixel of no class -- a false positive of whatever class is predicted there, nothing else.
A class enters an image's metrics only when it is present in that image's label map (tp + fn > 0); per present (image, class),
with HW pixels and tn = HW - tp - fp - fn (misc2.py at nan_for_nonexisting=False):
    dice = 2 tp / (2 tp + fp + fn)         jaccard = tp / (tp + fp + fn)        recall = tp / (tp + fn)
    precision = 0 if tp + fp == 0 else tp / (tp + fp)                          (the class is never predicted: zero by rule)
    f_measure = 2 precision recall / (precision + recall + 1e-5)
    specificity = 0 if tp + fn == HW else tn / (tn + fp)                       (the image is all this class: zero by rule)
`state[c] = [sum of each of the six over the (image, class c) pairs seen, their number]`, fp64, added in image order: additive
across batches and ranks (all_reduce it), and bit-repeatable -- the counts are integers and nothing is added atomically."""
import torch

from . import _lib
from ._lib import ITYPE

_TTYPE = {torch.int64: 0, torch.uint8: 1}
METRICS = ("dice", "jaccard", "precision", "recall", "f_measure", "specificity")


def supported(logits, targets, num_classes):
    if not (torch.is_tensor(logits) and torch.is_tensor(targets) and logits.is_cuda and targets.is_cuda
            and logits.device == targets.device):
        return False
    if not (logits.dim() == 4 and logits.dtype in ITYPE and targets.dim() == 3 and targets.dtype in _TTYPE):
        return False
    N, C, H, W = logits.shape
    if not (C == num_classes and 2 <= C <= 8 and N > 0 and 0 < H * W < 2 ** 31 and N * 64 < 2 ** 31):
        return False
    if tuple(targets.shape) != (N, H, W):
        return False
    return (logits.stride(3) == 1 and logits.stride(2) == W and targets.stride(2) == 1 and targets.stride(1) == W)


def _eager_counts(logits, targets, num_classes, return_preds):
    """The definition as torch ops: argmax over the classes, comparisons with the class index, integer sums."""
    pred = logits.argmax(dim=1)                                                       # (N, H, W)
    classes = torch.arange(num_classes, device=logits.device).view(1, -1, 1, 1)
    is_p, is_t = pred[:, None] == classes, targets[:, None].long() == classes         # (N, C, H, W) bool
    tp = (is_p & is_t).sum(dim=(2, 3))
    counts = torch.stack((tp, is_p.sum(dim=(2, 3)) - tp, is_t.sum(dim=(2, 3)) - tp), dim=-1).to(torch.int32)
    return (counts, pred.to(torch.uint8)) if return_preds else counts


def _eager_accumulate(state, counts, pixels):
    """state[c] += the six metrics and 1, for every image in order and every class present in it (fp64)."""
    tp, fp, fn = counts.to(torch.float64).unbind(-1)                                  # (N, C) each
    tn = pixels - tp - fp - fn
    zero = torch.zeros_like(tp)
    prec = torch.where(tp + fp == 0, zero, tp / (tp + fp))
    rec = tp / (tp + fn)
    vals = torch.stack((2.0 * tp / (2 * tp + fp + fn), tp / (tp + fp + fn), prec, rec,
                        2.0 * prec * rec / (prec + rec + 1e-5), torch.where(tp + fn == pixels, zero, tn / (tn + fp)),
                        torch.ones_like(tp)), dim=-1)                                 # (N, C, 7)
    vals = torch.where((tp + fn > 0)[..., None], vals, zero[..., None])              # absent classes: 0 / 0 above, dropped here
    for n in range(vals.shape[0]):
        state += vals[n]


def _run(logits, targets, return_preds, state):
    N, C, H, W = logits.shape
    dev = logits.device
    P = _lib.SegMetricsParams()
    P.batch, P.classes, P.pixels, P.itype, P.ttype = N, C, H * W, ITYPE[logits.dtype], _TTYPE[targets.dtype]
    P.logits_batch_stride, P.logits_c_stride, P.target_batch_stride = logits.stride(0), logits.stride(1), targets.stride(0)
    P.logits, P.target = logits.data_ptr(), targets.data_ptr()
    ws_bytes, ws = _lib.workspace("vivim_seg_metrics_workspace_bytes", P, dev)
    counts = _lib.empty((N, C, 3), torch.int32, dev)
    pred = _lib.empty((N, H, W), torch.uint8, dev) if return_preds else None
    P.workspace, P.workspace_bytes, P.counts = _lib.ptr(ws), ws_bytes, counts.data_ptr()
    if pred is not None:
        P.pred, P.pred_batch_stride = pred.data_ptr(), H * W
    if state is not None:
        P.state = state.data_ptr()
    _lib.launch("vivim_seg_metrics", P, dev)
    return (counts, pred) if return_preds else counts


def seg_confusion_counts(logits, targets, num_classes, return_preds=False):
    """int32 (N, C, 3) = {tp, fp, fn} of argmax(logits) against targets per (image, class), and with `return_preds` the uint8
    (N, H, W) prediction map: through the kernels where `supported` says so, as the eager composition otherwise."""
    logits = logits.detach()
    if not supported(logits, targets, num_classes):
        return _eager_counts(logits, targets, num_classes, return_preds)
    return _run(logits, targets, return_preds, None)


class SegMetricsTracker:
    """The reference's MulticlassMetricsTracker (final_multiclass_training.py:63-178) with its sums kept on the device: per class
    the mean of six metrics over the images whose label map holds the class.  `state` is the (C, 7) fp64 tensor of the sums and
    the number of (image, class) pairs; it lives where the first update's logits live."""

    def __init__(self, num_classes=3):
        self.num_classes = num_classes
        self.reset()

    def reset(self):
        self.state = torch.zeros(self.num_classes, 7, dtype=torch.float64)
        self._fresh = True

    def update(self, logits, targets):
        C = self.num_classes
        logits = logits.detach()
        if logits.dim() == 5:                                 # (B, T, C, H, W) / (B, T, H, W), as the validation step flattens them
            logits, targets = logits.flatten(0, 1), targets.flatten(0, 1)
        assert logits.dim() == 4 and logits.shape[1] == C and targets.dim() == 3, (tuple(logits.shape), tuple(targets.shape))
        if self.state.device != logits.device:
            # a fresh state is zeros: made on the device by a fill, not copied there
            self.state = torch.zeros_like(self.state, device=logits.device) if self._fresh else self.state.to(logits.device)
        self._fresh = False
        if logits.shape[0] == 0:
            return
        if supported(logits, targets, C) and self.state.is_contiguous():
            _run(logits, targets, False, self.state)
        else:
            _eager_accumulate(self.state, _eager_counts(logits, targets, C, False), logits.shape[2] * logits.shape[3])

    def get_results(self):
        st = self.state.cpu().tolist()                        # the one copy to the host
        counts = [int(row[6]) for row in st]
        out = {}
        for j, name in enumerate(METRICS):
            per_class = [st[c][j] / counts[c] if counts[c] > 0 else None for c in range(self.num_classes)]
            valid = [v for v in per_class if v is not None]
            out[name] = {"per_class": per_class, "mean": sum(valid) / len(valid) if valid else 0.0}
        out["class_counts"] = counts
        return out
