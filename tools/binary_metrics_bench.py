"""Validation metrics of the binary recipe: the device tracker (vivim_amd/binary_metrics.py, csrc/binary_metrics.hip) against a
reference-style host path, in one warmed process.
    python tools/binary_metrics_bench.py [--batches 20] [--rounds 7] [--host-batches 1] [--large-rounds 3] [--shape small|large|both] [--kernels-only]
Binarised predictions `(sigmoid(logits) > 0.5).float()` and float masks, (15, 1, 256, 256) and (40, 1, 512, 512) in fp32, already on
the device.  An epoch of the device path is `--batches` tracker updates and one get_results(); wall time between two device
synchronisations, divided by the batches.  The host path is the reference's `on_validation_epoch_end` restated from the definition:
per image three `.cpu().numpy()` copies of the map and the mask for S-measure, E-measure and MAE, then 256 thresholds, each
binarising on the device, copying both maps to the host and counting in numpy.  It is several thousand times slower, so an epoch of
it is `--host-batches` batches (wall time per batch is reported for both); the two paths alternate round by round and the median
round is given with the fastest and the slowest beside it (`--large-rounds` rounds at the large shape).  Launches are counted at the
C ABI (one call = five kernels, four without a state), bytes to the host by the tensors that `.cpu()` is called on.
--kernels-only: five updates at the chosen shapes and nothing else, for a counters-free
`rocprofv3 --kernel-trace --stats -- python tools/binary_metrics_bench.py --kernels-only --shape small`.
The yardstick is the host path of the same run."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(15, 256), (40, 512)]
EPS = np.spacing(1)
COPIED = [0, 0]                              # tensors copied to the host, their bytes


def to_host(t):
    COPIED[0] += 1
    COPIED[1] += t.numel() * t.element_size()
    return t.detach().cpu().numpy()


def make_batch(n, edge, dev, seed):
    """A blob mask per image and a noisy logit map around it, binarised as the validation step does."""
    g = torch.Generator().manual_seed(seed)
    rows, cols = torch.meshgrid(torch.arange(edge), torch.arange(edge), indexing="ij")
    c = torch.rand(n, 2, generator=g) * 0.5 + 0.25
    r = torch.rand(n, 2, generator=g) * 0.25 + 0.1
    mask = (((rows[None] / edge - c[:, :1, None]) / r[:, :1, None]) ** 2 + ((cols[None] / edge - c[:, 1:, None]) / r[:, 1:, None]) ** 2) <= 1.0
    logits = 3.0 * (mask.float() - 0.5) + 2.0 * torch.randn(n, edge, edge, generator=g)
    pred = (torch.sigmoid(logits) > 0.5).float()
    return pred[:, None].to(dev), mask.float()[:, None].to(dev)


def _ssim(x, t):
    n = x.size
    mx, my = x.mean(), t.mean()
    sx, sy, sxy = ((x - mx) ** 2).sum() / (n - 1), ((t - my) ** 2).sum() / (n - 1), ((x - mx) * (t - my)).sum() / (n - 1)
    alpha, beta = 4 * mx * my * sxy, (mx * mx + my * my) * (sx + sy)
    return alpha / (beta + EPS) if alpha != 0 else (1.0 if beta == 0 else 0.0)


def _prepare(pred, gt):
    gt = gt > 0.5
    if pred.max() != pred.min():
        pred = (pred - pred.min()) / (pred.max() - pred.min())
    return pred, gt


def host_smeasure(pred, gt):
    pred, g = _prepare(pred, gt)
    p = pred.astype(np.float64)
    y = g.mean()
    if y == 0:
        return 1 - p.mean()
    if y == 1:
        return p.mean()
    fg, bg = p[g], 1 - p[~g]
    obj = y * 2 * fg.mean() / (fg.mean() ** 2 + 1 + fg.std(ddof=1) + EPS) + (1 - y) * 2 * bg.mean() / (bg.mean() ** 2 + 1 + bg.std(ddof=1) + EPS)
    H, W = g.shape
    cy, cx = np.argwhere(g).mean(axis=0).round()
    X, Y = int(cx) + 1, int(cy) + 1
    t = g.astype(np.float64)
    w1, w2, w3 = X * Y / g.size, Y * (W - X) / g.size, (H - Y) * X / g.size
    region = (w1 * _ssim(p[:Y, :X], t[:Y, :X]) + w2 * _ssim(p[:Y, X:], t[:Y, X:]) + w3 * _ssim(p[Y:, :X], t[Y:, :X])
              + (1 - w1 - w2 - w3) * _ssim(p[Y:, X:], t[Y:, X:]))
    sm = 0.5 * obj + 0.5 * region
    return sm if sm > 0 else 0.0


def host_emeasure(pred, gt):
    pred, g = _prepare(pred, gt)
    S, G = g.size, int(g.sum())
    e = (pred * 255).astype(np.uint8)
    bins = np.linspace(0, 256, 257)
    fg_fg = np.cumsum(np.flip(np.histogram(e[g], bins=bins)[0])).astype(np.float64)
    fg_bg = np.cumsum(np.flip(np.histogram(e[~g], bins=bins)[0])).astype(np.float64)
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
        enhanced = 0.0
        for k, (a, c) in enumerate(((1 - mp, 1 - mg), (1 - mp, 0 - mg), (0 - mp, 1 - mg), (0 - mp, 0 - mg))):
            enhanced = enhanced + (2 * (a * c) / (a ** 2 + c ** 2 + EPS) + 1) ** 2 / 4 * numel[k]
    return float(np.mean(enhanced / (S - 1 + EPS)))


def host_mae(pred, gt):
    pred, g = _prepare(pred, gt)
    return float(np.mean(np.abs(pred.astype(np.float64) - g)))


def host_sweep(pred, gt, thresholds):
    """The 256-iteration loop: binarise on the device, copy both maps, count on the host."""
    gt_i = (gt > 0.5).to(int)
    sums = [0.0] * 6
    for t in thresholds:
        test, ref = to_host((pred > t).to(int)), to_host(gt_i)
        tp = int(((test != 0) * (ref != 0)).sum())
        fp = int(((test != 0) * (ref == 0)).sum())
        tn = int(((test == 0) * (ref == 0)).sum())
        fn = int(((test == 0) * (ref != 0)).sum())
        test_empty, ref_empty, ref_full = not np.any(test), not np.any(ref), bool(np.all(ref))
        prec = 0.0 if test_empty else tp / (tp + fp)
        rec = 0.0 if ref_empty else tp / (tp + fn)
        six = (0.0 if test_empty and ref_empty else 2.0 * tp / (2 * tp + fp + fn), 0.0 if test_empty and ref_empty else tp / (tp + fp + fn),
               prec, rec, 2 * prec * rec / (prec + rec + 1e-5), 0.0 if ref_full else tn / (tn + fp))
        for k in range(6):
            sums[k] += six[k]
    return [s / 256 for s in sums]


class HostPath:
    """The reference's loop over (pred, gt) pairs of one image each, with the tracker's surface."""

    def __init__(self):
        self.thresholds = np.linspace(1, 0, 256)
        self.rows = []

    def update(self, pred, gt):
        for n in range(pred.shape[0]):
            p, g = pred[n, 0], gt[n, 0]
            with np.errstate(all="ignore"):
                sm = host_smeasure(to_host(p), to_host(g))
            em = host_emeasure(to_host(p), to_host(g))
            mae = host_mae(to_host(p), to_host(g))
            self.rows.append(host_sweep(p, g, self.thresholds) + [sm, em, mae])

    def get_results(self):
        from vivim_amd.binary_metrics import VALUES
        mean = np.mean(np.array(self.rows, dtype=np.float64), axis=0)
        return dict(zip(VALUES, mean.tolist()))


def epoch(make_tracker, batches):
    """Seconds per batch of one epoch: updates, then get_results, between two device synchronisations."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tracker = make_tracker()
    for pred, gt in batches:
        tracker.update(pred, gt)
    res = tracker.get_results()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(batches), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-batches", type=int, default=1)
    ap.add_argument("--large-rounds", type=int, default=3)
    ap.add_argument("--shape", choices=("small", "large", "both"), default="both")
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    from vivim_amd import _lib
    from vivim_amd.binary_metrics import BinaryMetricsTracker, VALUES
    dev = torch.device("cuda:0")
    shapes = {"small": SHAPES[:1], "large": SHAPES[1:], "both": SHAPES}[args.shape]
    calls = []
    real_call = _lib.call
    _lib.call = lambda name, P, stream, *extra: (calls.append(name), real_call(name, P, stream, *extra))[1]

    if args.kernels_only:
        for n, edge in shapes:
            pred, gt = make_batch(n, edge, dev, 1)
            tracker = BinaryMetricsTracker()
            for _ in range(5):
                tracker.update(pred, gt)
            print(f"({n}, 1, {edge}, {edge}): 5 updates, Dice {tracker.get_results()['Dice']:.6f}")
        return

    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    for (n, edge) in shapes:
        rounds = args.rounds if edge <= 256 else args.large_rounds
        batches = [make_batch(n, edge, dev, 100 + i) for i in range(4)]
        batches = [batches[i % 4] for i in range(args.batches)]
        host_batches = batches[:args.host_batches]
        epoch(BinaryMetricsTracker, batches)                                         # warm-up: library, code objects, allocator blocks
        epoch(BinaryMetricsTracker, batches)
        HostPath().update(batches[0][0][:1], batches[0][1][:1])
        times = {"device": [], "host": []}
        for _ in range(rounds):
            calls.clear()
            t, res_dev = epoch(BinaryMetricsTracker, batches)
            times["device"].append(t)
            n_calls = len(calls)
            COPIED[:] = [0, 0]
            t, res_host = epoch(HostPath, host_batches)
            times["host"].append(t)
            copied = tuple(COPIED)
        one = BinaryMetricsTracker()                                                  # the same batches as the host path, for the numbers
        for pred, gt in host_batches:
            one.update(pred, gt)
        res_one = one.get_results()
        worst = max(abs(res_one[k] - res_host[k]) for k in VALUES)
        print(f"\n({n}, 1, {edge}, {edge}) fp32, {rounds} rounds; device: {args.batches} batches per epoch, host: {len(host_batches)}")
        med = {}
        for k, v in times.items():
            med[k] = statistics.median(v)
            print(f"    {k:8s} {med[k] * 1e3:12.3f} ms per batch  (min {min(v) * 1e3:.3f}, max {max(v) * 1e3:.3f})")
        print(f"    host / device: {med['host'] / med['device']:.0f} x")
        print(f"    device: {n_calls} C-ABI calls per epoch = {5 * n_calls} kernel launches ({5} per batch), 80 bytes to the host per epoch")
        print(f"    host:   {copied[0] // len(host_batches)} copies and {copied[1] / len(host_batches) / 2 ** 20:.1f} MiB to the host per batch "
              f"({copied[0] // (len(host_batches) * n)} copies per image)")
        print(f"    the nine means of the two paths over the host path's batches differ by at most {worst:.3e}")
        print("    " + ", ".join(f"{k} {res_dev[k]:.4f}" for k in VALUES))


if __name__ == "__main__":
    main()
