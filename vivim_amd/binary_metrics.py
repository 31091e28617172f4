"""Validation metrics of the binary (one-channel) recipe on the device (csrc/binary_metrics.hip;
include/vivim_hip_ext_binary_metrics.h): what the reference's `on_validation_epoch_end` of its binary training script logs -- the
256-threshold sweep of six confusion metrics, S-measure, mean E-measure and MAE -- without moving a map to the host.

    binary_image_metrics(pred, gt, return_hist=False) -> fp64 (N, 9) [, int32 (N, 4, 256)]
    supported(pred, gt)                      whether the kernels take these tensors; where they do not (CPU tensors, other layouts,
                                             other dtypes) the same definition runs as an eager torch composition in fp64
    BinaryMetricsTracker()                   reset() / update(pred, gt) / get_results(); update() launches five kernels and neither
                                             synchronises nor copies anything to the host, get_results() copies the (10,) fp64
                                             `state` once

Inputs.  pred (N, H, W), (N, 1, H, W) or (B, T, 1, H, W), fp32 / fp16 / bf16 (widened to fp32 exactly: everything below is on the
fp32 value p), rows contiguous, taken as handed over (probabilities, or an already binarised map).  gt of the same shape: a float
type (g = gt > 0.5) or uint8 / bool (g = gt != 0).  H * W >= 2.  A NaN in pred is outside the definition: nothing faults, the result
is unspecified.

Per image nine values, in the order of VALUES, in fp64 unless said otherwise.  S = H * W, G = |g|.
  Sweep (Dice, Jaccard, Precision, Recall, Fmeasure, specificity), on the raw p.  t_j = float32(numpy.linspace(1, 0, 256)[j]);
    test_j = p > t_j, strictly, in fp32.  With the integers tp, fp, fn, tn of test_j against g (misc2.py's rules at
    nan_for_nonexisting=False): dice = 2tp / (2tp + fp + fn) and jaccard = tp / (tp + fp + fn), 0 when test_j and g are both empty;
    precision = tp / (tp + fp), 0 when test_j is empty; recall = tp / (tp + fn), 0 when g is empty; f = 2 prec rec / (prec + rec +
    1e-5); specificity = tn / (tn + fp), 0 when g is full.  Each value is the sum over j = 0..255 divided by 256.
  Normalisation.  mn, mx = min, max of p over the image; pn = (p - mn) / (mx - mn) as two correctly rounded fp32 operations when
    mx != mn, pn = p otherwise.
  MAE = mean |pn - g|.
  Emeasure.  e = uint8(pn * 255): an fp32 product, truncated, clamped to [0, 255] (the clamp acts only on a constant map outside
    [0, 1], where numpy's cast is undefined).  256-bin histograms of e over g and over ~g; their flipped cumulative sums are fg_fg
    and fg_bg per threshold.  The enhanced sum is the predicted-background count when G == 0, the predicted-foreground count when
    G == S, else the sum over the four (predicted, true) parts of ((2ab / (a^2 + b^2 + eps) + 1)^2 / 4) * part size with a, b the
    demeaned values of the part; em_k = sum_k / (S - 1 + eps), eps = numpy.spacing(1); the value is the mean over k.
  Smeasure (alpha = 0.5), on pn and g.  y = G / S.  y == 0: 1 - mean(pn); y == 1: mean(pn); else max(0, 0.5 object + 0.5 region).
    object = y s_obj(pn over g) + (1 - y) s_obj(1 - pn over ~g), s_obj = 2x / (x^2 + 1 + sigma + eps) with the mean x and the sample
    standard deviation sigma (ddof = 1).  region: the centroid is (rint(sum of columns / G) + 1, rint(sum of rows / G) + 1) =
    (X, Y), integer sums, round-half-even; the map is cut into four quadrants at column X and row Y with the weights X Y / S,
    (W - X) Y / S, X (H - Y) / S and 1 minus the three; each quadrant scores alpha / (beta + eps) when alpha != 0, else 1 when
    beta == 0, else 0, where alpha = 4 x y sxy, beta = (x^2 + y^2)(sx + sy) with the quadrant's means x, y of pn, g and their
    variances and covariance over n - 1.  Means first, then centred second moments, in fp64: a quadrant where pn is constant
    has exactly sx = sxy = 0.
    WHERE THE REFERENCE'S ARITHMETIC YIELDS NaN THE IMAGE'S S-MEASURE IS 0 (what its max(0, nan) returns): a quadrant of fewer
    than 2 pixels (a centroid in the last row or column leaves one empty: X == W or Y == H), G == 1, or S - G == 1.

Tracker.  `state` is fp64 (10,): the sums of the nine values over the images seen, added in image order, and the image count.
Additive across batches and ranks (all_reduce it) and bit-repeatable: the device path has no float atomics and adds its partial
sums in a fixed order.  get_results() returns the nine means under the names the reference logs."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import ITYPE, BinaryMetricsParams

VALUES = ("Dice", "Jaccard", "Precision", "Recall", "Fmeasure", "specificity", "Smeasure", "Emeasure", "MAE")
_GTYPE = {**ITYPE, torch.uint8: 3, torch.bool: 3}
_EPS = float(np.spacing(1))
_thresholds = {}


def thresholds(device):
    """float32(numpy.linspace(1, 0, 256)) on `device`: made on the host once per device, never recomputed there."""
    key = str(device)
    if key not in _thresholds:
        _thresholds[key] = torch.from_numpy(np.linspace(1, 0, 256).astype(np.float32)).to(device)
    return _thresholds[key]


def _flatten(pred, gt):
    """-> (N, H, W) views of pred and gt, whichever of the three shapes they came in."""
    assert pred.shape == gt.shape, (tuple(pred.shape), tuple(gt.shape))
    if pred.dim() == 5:
        pred, gt = pred.flatten(0, 1), gt.flatten(0, 1)
    if pred.dim() == 4:
        assert pred.shape[1] == 1, tuple(pred.shape)
        pred, gt = pred[:, 0], gt[:, 0]
    assert pred.dim() == 3 and (pred.shape[0] == 0 or pred.shape[1] * pred.shape[2] >= 2), tuple(pred.shape)
    return pred, gt


def _supported3(pred, gt):
    if not (pred.is_cuda and gt.is_cuda and pred.device == gt.device and pred.dtype in ITYPE and gt.dtype in _GTYPE):
        return False
    N, H, W = pred.shape
    if not (N > 0 and 2 <= H * W <= 2 ** 31 - 1 - 4096 and N * 32 < 2 ** 31):
        return False
    return all(t.stride(2) == 1 and t.stride(1) == W and t.stride(0) >= H * W for t in (pred, gt))


def supported(pred, gt):
    if not (torch.is_tensor(pred) and torch.is_tensor(gt) and pred.shape == gt.shape and pred.dim() in (3, 4, 5)):
        return False
    if (pred.dim() != 3 and pred.shape[-3] != 1) or pred.shape[-2] * pred.shape[-1] < 2:
        return False
    pred, gt = _flatten(pred, gt)
    return _supported3(pred, gt)


def _eager(pred, gt, return_hist):
    """The definition of the module docstring as torch ops, on whatever device the tensors live: (N, H, W) -> fp64 (N, 9)."""
    p = pred.float()
    g = gt != 0 if gt.dtype in (torch.uint8, torch.bool) else gt.float() > 0.5
    N, H, W = p.shape
    S, dev, f64 = H * W, p.device, torch.float64
    pf, gf = p.reshape(N, S), g.reshape(N, S)
    G = gf.sum(1)                                                                     # int64 (N,)
    # the sweep bin: how many thresholds p exceeds = how many of the ascending table lie strictly below p, compared in fp32
    b = torch.searchsorted(thresholds(dev).flip(0).contiguous(), pf.contiguous(), right=False)
    mn, mx = pf.min(1, keepdim=True).values, pf.max(1, keepdim=True).values
    norm = mx != mn
    pn = torch.where(norm, (pf - mn) / torch.where(norm, mx - mn, torch.ones_like(mx)), pf)
    e = (pn * 255.0).clamp(0.0, 255.0).to(torch.int64)                                # truncation
    image = torch.arange(N, device=dev)[:, None]
    hist = torch.zeros(N, 4, 257, dtype=torch.int64, device=dev)
    hist.view(-1).index_add_(0, ((image * 4 + torch.where(gf, 0, 1)) * 257 + b).view(-1), torch.ones(N * S, dtype=torch.int64, device=dev))
    hist.view(-1).index_add_(0, ((image * 4 + torch.where(gf, 2, 3)) * 257 + e + 1).view(-1), torch.ones(N * S, dtype=torch.int64, device=dev))
    hist = hist[:, :, 1:]                                                              # the sweep's bin 0 enters no count
    cum = hist.flip(-1).cumsum(-1).to(f64)                                             # (N, 4, 256), per threshold
    Gd, Sd = G.to(f64)[:, None], float(S)
    zero = torch.zeros(N, 256, dtype=f64, device=dev)

    tp, fp = cum[:, 0], cum[:, 1]
    fn, tn = Gd - tp, (Sd - Gd) - fp
    test_empty, ref_empty, ref_full = tp + fp == 0, (Gd == 0).expand(N, 256), (Gd == Sd).expand(N, 256)
    prec = torch.where(test_empty, zero, tp / (tp + fp))
    rec = torch.where(ref_empty, zero, tp / (tp + fn))
    sweep = [torch.where(test_empty & ref_empty, zero, 2.0 * tp / (2.0 * tp + fp + fn)),
             torch.where(test_empty & ref_empty, zero, tp / (tp + fp + fn)), prec, rec,
             2.0 * prec * rec / (prec + rec + 1e-5), torch.where(ref_full, zero, tn / (tn + fp))]

    fg_fg, fg_bg = cum[:, 2], cum[:, 3]
    pred_fg = fg_fg + fg_bg
    pred_bg = Sd - pred_fg
    bg_fg = Gd - fg_fg
    numel = (fg_fg, fg_bg, bg_fg, pred_bg - bg_fg)
    mp, mg = pred_fg / Sd, (Gd / Sd).expand(N, 256)
    parts = torch.zeros_like(zero)
    for k, (a, c) in enumerate(((1.0 - mp, 1.0 - mg), (1.0 - mp, 0.0 - mg), (0.0 - mp, 1.0 - mg), (0.0 - mp, 0.0 - mg))):
        align = 2.0 * (a * c) / (a * a + c * c + _EPS)
        parts = parts + (align + 1.0) ** 2 / 4.0 * numel[k]
    em = torch.where(ref_empty, pred_bg, torch.where(ref_full, pred_fg, parts)) / (Sd - 1.0 + _EPS)

    pd, gd = pn.to(f64), gf.to(f64)
    mae = (pd - gd).abs().sum(1) / Sd

    # S-measure.  Divisions by zero give NaN here as in the reference; the NaN becomes 0 at the end.
    Gs, Bs = G.to(f64), Sd - G.to(f64)
    xf, xb = (pd * gd).sum(1) / Gs, ((1.0 - pd) * (1.0 - gd)).sum(1) / Bs
    sf = ((((pd - xf[:, None]) ** 2) * gd).sum(1) / (Gs - 1.0)).sqrt()
    sb = (((((1.0 - pd) - xb[:, None]) ** 2) * (1.0 - gd)).sum(1) / (Bs - 1.0)).sqrt()
    y = Gs / Sd
    obj = y * (2.0 * xf / (xf * xf + 1.0 + sf + _EPS)) + (1.0 - y) * (2.0 * xb / (xb * xb + 1.0 + sb + _EPS))
    rows = torch.arange(H, device=dev).repeat_interleave(W)[None, :]                   # (1, S)
    cols = torch.arange(W, device=dev).repeat(H)[None, :]
    some = G > 0
    safe = torch.where(some, Gs, torch.ones_like(Gs))
    X = torch.where(some, (gf * cols).sum(1).to(f64) / safe, torch.full_like(Gs, W / 2)).round().to(torch.int64).clamp(0, W - 1) + 1
    Y = torch.where(some, (gf * rows).sum(1).to(f64) / safe, torch.full_like(Gs, H / 2)).round().to(torch.int64).clamp(0, H - 1) + 1
    Xd, Yd = X.to(f64), Y.to(f64)
    sizes = (Xd * Yd, (W - Xd) * Yd, Xd * (H - Yd), (W - Xd) * (H - Yd))
    weights = [sizes[0] / Sd, sizes[1] / Sd, sizes[2] / Sd]
    weights.append(1.0 - weights[0] - weights[1] - weights[2])
    region = torch.zeros_like(Gs)
    for q in range(4):
        inside = ((rows >= Y[:, None]) == bool(q & 2)) & ((cols >= X[:, None]) == bool(q & 1))
        m, n = inside.to(f64), sizes[q]
        x, yq = (pd * m).sum(1) / n, (gd * m).sum(1) / n
        dx, dy = pd - x[:, None], gd - yq[:, None]
        sx, sy, sxy = (dx * dx * m).sum(1) / (n - 1.0), (dy * dy * m).sum(1) / (n - 1.0), (dx * dy * m).sum(1) / (n - 1.0)
        alpha, beta = 4.0 * x * yq * sxy, (x * x + yq * yq) * (sx + sy)
        score = torch.where(alpha != 0, alpha / (beta + _EPS), torch.where(beta == 0, torch.ones_like(beta), torch.zeros_like(beta)))
        region = region + weights[q] * score
    sm = 0.5 * obj + 0.5 * region
    sm = torch.where(sm > 0, sm, torch.zeros_like(sm))                                 # max(0, sm), and 0 for a NaN
    mean_pn = pd.sum(1) / Sd
    sm = torch.where(G == 0, 1.0 - mean_pn, torch.where(G == S, mean_pn, sm))

    values = torch.stack([v.sum(1) / 256.0 for v in sweep] + [sm, em.sum(1) / 256.0, mae], dim=1)
    return (values, hist.to(torch.int32)) if return_hist else values


def _run(pred, gt, return_hist, state):
    N, H, W = pred.shape
    dev = pred.device
    P = BinaryMetricsParams()
    P.struct_bytes = ctypes.sizeof(P)
    P.batch, P.height, P.width, P.ptype, P.gtype = N, H, W, ITYPE[pred.dtype], _GTYPE[gt.dtype]
    P.pred_batch_stride, P.gt_batch_stride = pred.stride(0), gt.stride(0)
    P.pred, P.gt, P.thresholds = pred.data_ptr(), gt.data_ptr(), thresholds(dev).data_ptr()
    ws_bytes, ws = _lib.workspace("vivim_binary_metrics_workspace_bytes", P, dev)
    _lib.check(ws_bytes > 0, "vivim_binary_metrics_workspace_bytes refused the shapes")
    values = _lib.empty((N, 9), torch.float64, dev)
    hist = _lib.empty((N, 4, 256), torch.int32, dev) if return_hist else None
    P.values, P.hist, P.workspace, P.workspace_bytes = values.data_ptr(), _lib.ptr(hist), _lib.ptr(ws), ws_bytes
    if state is not None:
        P.state = state.data_ptr()
    _lib.launch("vivim_binary_metrics", P, dev)
    return (values, hist) if return_hist else values


def binary_image_metrics(pred, gt, return_hist=False):
    """fp64 (N, 9), the nine values of VALUES per image, and with `return_hist` the int32 (N, 4, 256) histograms (the sweep's over g
    and over ~g, bin i = the pixels that exceed exactly i + 1 thresholds; then the E-measure's two): through the kernels where
    `supported` says so, as the eager composition otherwise."""
    pred, gt = _flatten(pred.detach(), gt)
    if pred.shape[0] == 0:
        values = torch.zeros(0, 9, dtype=torch.float64, device=pred.device)
        return (values, torch.zeros(0, 4, 256, dtype=torch.int32, device=pred.device)) if return_hist else values
    if _supported3(pred, gt):
        return _run(pred, gt, return_hist, None)
    return _eager(pred, gt, return_hist)


class BinaryMetricsTracker:
    """The nine numbers the reference's binary validation logs (complements/train_binary.py:205-282), their sums kept on the device.
    `state` is the (10,) fp64 tensor of the sums and the image count; it lives where the first update's maps live."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.state = torch.zeros(10, dtype=torch.float64)
        self._fresh = True

    def update(self, pred, gt):
        pred, gt = _flatten(pred.detach(), gt)
        if self.state.device != pred.device:
            # a fresh state is zeros: made on the device by a fill, not copied there
            self.state = torch.zeros_like(self.state, device=pred.device) if self._fresh else self.state.to(pred.device)
        self._fresh = False
        if pred.shape[0] == 0:
            return
        if _supported3(pred, gt) and self.state.is_contiguous():
            _run(pred, gt, False, self.state)
        else:
            values = _eager(pred, gt, False)
            for n in range(values.shape[0]):
                self.state[:9] += values[n]
            self.state[9] += values.shape[0]

    def get_results(self):
        st = self.state.cpu().tolist()                        # the one copy to the host
        count = st[9]
        return {name: (st[k] / count if count > 0 else 0.0) for k, name in enumerate(VALUES)}
