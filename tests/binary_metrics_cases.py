"""What the binary-metrics tests share (no test in here): the definition of vivim_amd/binary_metrics.py's docstring restated as
plain numpy fp64 (`restate64`), a second evaluation of the same whose sums are math.fsum sums (`restate_exact`: the distance
between the two says how ill-conditioned an image's S-measure is), the fixtures, and the generator of further inputs.

The reference computes MAE and S-measure in fp32, so the fixtures' values of those two differ from the fp64 restatement.  Measured
on the CPU over the committed fixtures (tests/golden/make_golden_binary_metrics.py prints it), the largest |reference -
restate64| is REFERENCE_FP32_GAP below; the CPU test allows 4 times that."""
import glob
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VALUES = ("Dice", "Jaccard", "Precision", "Recall", "Fmeasure", "specificity", "Smeasure", "Emeasure", "MAE")
THRESHOLDS = np.linspace(1, 0, 256).astype(np.float32)
EPS = np.spacing(1)
REFERENCE_FP32_GAP = {"MAE": 3.98e-8, "Smeasure": 3.36e-8}       # measured: 3.9753e-08 and 3.3539e-08, rounded up


def _sum64(a):
    return float(np.sum(np.asarray(a, dtype=np.float64)))


def _sum_exact(a):
    return math.fsum(np.asarray(a, dtype=np.float64).ravel().tolist())


def normalise(p):
    p = np.asarray(p, dtype=np.float32)
    mn, mx = p.min(), p.max()
    return (p - mn) / (mx - mn) if mx != mn else p            # fp32 array with fp32 scalars: two correctly rounded fp32 operations


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _smeasure(pn, g, total):
    H, W = g.shape
    S, G = H * W, int(g.sum())
    pd, gd = pn.astype(np.float64), g.astype(np.float64)
    if G == 0:
        return 1.0 - total(pd) / S
    if G == S:
        return total(pd) / S

    def s_obj(x):
        mean = total(x) / x.size
        sigma = math.sqrt(_div(total((x - mean) ** 2), x.size - 1)) if x.size != 1 else float("nan")
        return 2.0 * mean / (mean * mean + 1.0 + sigma + EPS)

    y = G / S
    obj = y * s_obj(pd[g]) + (1.0 - y) * s_obj(1.0 - pd[~g])
    rows, cols = np.nonzero(g)
    X, Y = int(np.rint(int(cols.sum()) / G)) + 1, int(np.rint(int(rows.sum()) / G)) + 1

    def ssim(x, t):
        n = x.size
        if n < 2:
            return float("nan")
        mx, my = total(x) / n, total(t) / n
        sx, sy, sxy = total((x - mx) ** 2) / (n - 1), total((t - my) ** 2) / (n - 1), total((x - mx) * (t - my)) / (n - 1)
        alpha, beta = 4.0 * mx * my * sxy, (mx * mx + my * my) * (sx + sy)
        return alpha / (beta + EPS) if alpha != 0 else (1.0 if beta == 0 else 0.0)

    w1, w2, w3 = X * Y / S, Y * (W - X) / S, (H - Y) * X / S
    w4 = 1.0 - w1 - w2 - w3
    region = (w1 * ssim(pd[:Y, :X], gd[:Y, :X]) + w2 * ssim(pd[:Y, X:], gd[:Y, X:]) + w3 * ssim(pd[Y:, :X], gd[Y:, :X])
              + w4 * ssim(pd[Y:, X:], gd[Y:, X:]))
    sm = 0.5 * obj + 0.5 * region
    return sm if sm > 0 else 0.0                              # max(0, sm); NaN: 0


def restate(pred, gt, total=_sum64):
    """One image: pred (H, W) fp32, gt (H, W) bool -> dict(values (9,), counts (256, 4) = tp, fp, fn, tn per threshold,
    sweep_fg / sweep_bg (256,) with bin i = pixels exceeding exactly i + 1 thresholds, e_fg / e_bg (256,))."""
    p, g = np.asarray(pred, dtype=np.float32), np.asarray(gt, dtype=bool)
    H, W = p.shape
    S, G = H * W, int(g.sum())
    counts = np.zeros((256, 4), dtype=np.int64)
    sums = [0.0] * 6
    for j, t in enumerate(THRESHOLDS):
        test = p > t                                           # fp32 against fp32, strictly
        tp, fp = int((test & g).sum()), int((test & ~g).sum())
        fn, tn = G - tp, S - G - fp
        counts[j] = (tp, fp, fn, tn)
        test_empty, ref_empty, ref_full = tp + fp == 0, G == 0, G == S
        prec = 0.0 if test_empty else tp / (tp + fp)
        rec = 0.0 if ref_empty else tp / (tp + fn)
        six = (0.0 if test_empty and ref_empty else 2.0 * tp / (2 * tp + fp + fn),
               0.0 if test_empty and ref_empty else tp / (tp + fp + fn), prec, rec,
               2.0 * prec * rec / (prec + rec + 1e-5), 0.0 if ref_full else tn / (tn + fp))
        for k in range(6):
            sums[k] += six[k]
    b = (p[..., None] > THRESHOLDS).sum(-1)
    sweep_fg, sweep_bg = np.bincount(b[g], minlength=257)[1:], np.bincount(b[~g], minlength=257)[1:]

    pn = normalise(p)
    mae = total(np.abs(pn.astype(np.float64) - g)) / S
    e = np.clip(np.trunc(pn * np.float32(255)), 0, 255).astype(np.int64)
    e_fg, e_bg = np.bincount(e[g], minlength=256), np.bincount(e[~g], minlength=256)
    fg_fg, fg_bg = np.cumsum(e_fg[::-1]).astype(np.float64), np.cumsum(e_bg[::-1]).astype(np.float64)
    pred_fg = fg_fg + fg_bg
    pred_bg = S - pred_fg
    if G == 0:
        enhanced = pred_bg
    elif G == S:
        enhanced = pred_fg
    else:
        bg_fg = G - fg_fg
        numel = (fg_fg, fg_bg, bg_fg, pred_bg - bg_fg)
        mp, mg = pred_fg / S, G / S
        enhanced = np.zeros(256)
        for k, (a, c) in enumerate(((1 - mp, 1 - mg), (1 - mp, 0 - mg), (0 - mp, 1 - mg), (0 - mp, 0 - mg))):
            align = 2 * (a * c) / (a ** 2 + c ** 2 + EPS)
            enhanced = enhanced + (align + 1) ** 2 / 4 * numel[k]
    em = total(enhanced / (S - 1 + EPS)) / 256
    with np.errstate(all="ignore"):
        sm = _smeasure(pn, g, total)
    values = np.array([s / 256 for s in sums] + [sm, em, mae], dtype=np.float64)
    return dict(values=values, counts=counts, sweep_fg=sweep_fg, sweep_bg=sweep_bg, e_fg=e_fg, e_bg=e_bg)


def restate64(pred, gt):
    return restate(pred, gt, _sum64)


def restate_exact(pred, gt):
    return restate(pred, gt, _sum_exact)


def counts_from_hist(hist, G, S):
    """(4, 256) histograms of one image -> the sweep's (256, 4) tp, fp, fn, tn and the E-measure's two histograms."""
    tp, fp = np.cumsum(hist[0][::-1].astype(np.int64)), np.cumsum(hist[1][::-1].astype(np.int64))
    return np.stack([tp, fp, G - tp, S - G - fp], axis=1), hist[2], hist[3]


def fixtures():
    """name -> dict of arrays, every tests/golden/binm_*.npz."""
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "binm_*.npz"))):
        with np.load(path) as z:
            out[os.path.basename(path)[5:-4]] = {k: z[k] for k in z.files}
    return out


def exact_in_16_bits(p):
    """Round a fp32 map in [0, 1] to values that bf16 and fp16 both hold exactly: 8 significant bits, nothing below 2^-10."""
    import torch
    t = torch.from_numpy(np.asarray(p, dtype=np.float32)).to(torch.bfloat16).to(torch.float32)
    t[t < 2.0 ** -10] = 0.0
    assert torch.equal(t.to(torch.float16).float(), t)
    return t.numpy()


def blob_mask(rng, n, h, w):
    """n masks (h, w) bool: an axis-aligned ellipse at a random place, neither empty nor full for h * w >= 12."""
    rows, cols = np.mgrid[0:h, 0:w]
    out = np.zeros((n, h, w), dtype=bool)
    for i in range(n):
        cy, cx = rng.uniform(0.25, 0.75) * h, rng.uniform(0.25, 0.75) * w
        ry, rx = rng.uniform(0.15, 0.4) * h + 0.6, rng.uniform(0.15, 0.4) * w + 0.6
        out[i] = ((rows - cy) / ry) ** 2 + ((cols - cx) / rx) ** 2 <= 1.0
    return out


def probability_maps(rng, gt):
    """A noisy, blurred-looking probability map per mask, exact in bf16 and fp16."""
    p = np.clip(0.65 * gt + 0.15 + 0.25 * rng.standard_normal(gt.shape), 0.0, 1.0)
    return exact_in_16_bits(p)


def make_inputs(shape, n, seed, binarised=False):
    """-> pred fp32 (n, h, w), gt bool (n, h, w): probability maps, or binarised ones, around random blobs."""
    rng = np.random.default_rng(seed)
    gt = blob_mask(rng, n, *shape)
    pred = probability_maps(rng, gt)
    return ((pred > 0.5).astype(np.float32) if binarised else pred), gt


def constant_quadrant(seed=7):
    """A (33, 70) probability map whose left-top quadrant holds no mask pixel and is a constant 0.3 (min 0 and max 1 lie elsewhere,
    so pn = 0.3f there): its sx and sxy must be exactly 0 and sy is, so the quadrant scores 1 by the `alpha == 0 and beta == 0`
    branch -- rounding noise in sx would make it 0 and move the S-measure by half the quadrant's weight, about 0.12.  The mask
    is two rectangles, top right and bottom left; the centroid depends on it alone: (X, Y) = (33, 17)."""
    rng = np.random.default_rng(seed)
    gt = np.zeros((1, 33, 70), dtype=bool)
    gt[0, 2:10, 45:65] = True
    gt[0, 20:30, 5:25] = True
    rows, cols = np.nonzero(gt[0])
    X, Y = int(np.rint(cols.sum() / len(cols))) + 1, int(np.rint(rows.sum() / len(rows))) + 1
    assert (X, Y) == (33, 17) and not gt[0, :Y, :X].any()
    pred = probability_maps(rng, gt)
    pred[0, -1, -1], pred[0, -1, -2] = 0.0, 1.0
    pred[0, :Y, :X] = np.float32(0.3)
    return pred, gt
