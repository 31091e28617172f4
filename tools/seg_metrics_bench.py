"""Validation metrics of a batch of logits, three ways in one warmed process, wall time with a device sync around the timed region:
  (a) device   SegMetricsTracker.update per batch (csrc/seg_metrics.hip) + one get_results() per epoch of --batches batches
  (b) host     the reference-style path: logits.float().cpu().numpy() (bf16 cannot go to numpy as it is), targets to the host,
               then a numpy loop over images x classes restated from the definition in vivim_amd/seg_metrics.py -- one argmax per
               image and one set of counts per (image, class), which is less work than the reference's tracker does (it takes the
               argmax once per class and the confusion matrix once per metric), so this yardstick flatters the host path
  (c) eager    the torch composition of the same definition on the device (seg_metrics._eager_counts + _eager_accumulate)
and the launches of one update (tools/launch_count.py's method) and the bytes each path copies to the host per batch.
    python tools/seg_metrics_bench.py [--batches 20] [--rounds 3] [--host-batches 3]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from launch_count import launches, show  # noqa: E402  (this directory: the script's own)

SHAPES = ((15, 3, 256, 256), (40, 3, 512, 512))          # the bench workload (batch 3 x clip 5); 512^2, batch 8 x clip 5


def host_update(sums, logits, targets, C):
    """The reference-style update: everything to the host, then numpy reductions per (image, class)."""
    x = logits.detach().float().cpu().numpy()
    t = targets.detach().cpu().numpy()
    HW = x.shape[2] * x.shape[3]
    for n in range(x.shape[0]):
        pred = x[n].argmax(axis=0)
        for c in range(C):
            gt_c = t[n] == c
            ng = int(gt_c.sum())
            if ng == 0:
                continue
            pred_c = pred == c
            tp = int((pred_c & gt_c).sum())
            fp, fn = int(pred_c.sum()) - tp, ng - tp
            tn = HW - tp - fp - fn
            prec = 0.0 if tp + fp == 0 else tp / (tp + fp)
            rec = tp / (tp + fn)
            sums[c] += np.array([2.0 * tp / (2 * tp + fp + fn), tp / (tp + fp + fn), prec, rec,
                                 2.0 * prec * rec / (prec + rec + 1e-5), 0.0 if tp + fn == HW else tn / (tn + fp), 1.0])


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-batches", type=int, default=3, help="batches timed for the host path per round (it is slow)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "seg_metrics_bench needs a GPU"
    dev = torch.device("cuda:0")
    from vivim_amd import seg_metrics
    for shape in SHAPES:
        N, C, H, W = shape
        g = torch.Generator().manual_seed(0)
        logits = (torch.randn(shape, generator=g) * 4).to(torch.bfloat16).to(dev)
        targets = torch.randint(0, C, (N, H, W), generator=g).to(dev)
        assert seg_metrics.supported(logits, targets, C)

        def device_epoch(n=a.batches):
            tr = seg_metrics.SegMetricsTracker(C)
            for _ in range(n):
                tr.update(logits, targets)
            return tr.get_results()

        def eager_epoch(n=a.batches):
            state = torch.zeros(C, 7, dtype=torch.float64, device=dev)
            for _ in range(n):
                seg_metrics._eager_accumulate(state, seg_metrics._eager_counts(logits, targets, C, False), H * W)
            return state.cpu()

        def host_epoch(n=a.host_batches):
            sums = np.zeros((C, 7))
            for _ in range(n):
                host_update(sums, logits, targets, C)
            return sums

        res, st_e, st_h = device_epoch(2), eager_epoch(2), host_epoch(1)           # warm all three, and check they agree
        for c in range(C):
            assert res["class_counts"][c] == int(st_e[c, 6]) == 2 * int(st_h[c, 6])
            assert abs(res["dice"]["per_class"][c] - st_h[c, 0] / st_h[c, 6]) < 1e-12
            assert abs(float(st_e[c, 0]) - 2 * st_h[c, 0]) < 1e-9
        t = {"device": [], "eager": [], "host": []}
        for _ in range(a.rounds):                                                   # alternate
            t["device"].append(wall(device_epoch) / a.batches)
            t["eager"].append(wall(eager_epoch) / a.batches)
            t["host"].append(wall(host_epoch) / a.host_batches)
        to_host = {"device": 0, "eager": 0, "host": N * C * H * W * 4 + N * H * W * 8}
        print(f"== metrics of one batch, logits {shape} bf16, int64 targets; per batch over epochs of {a.batches} batches "
              f"(host path: {a.host_batches}), {a.rounds} rounds alternating, wall time with device sync")
        for n in ("device", "host", "eager"):
            print(f"   {n:6s} median {statistics.median(t[n]) * 1e3:10.3f} ms / batch  min {min(t[n]) * 1e3:10.3f}  max {max(t[n]) * 1e3:10.3f}"
                  f"   to the host per batch {to_host[n] / 1e6:8.2f} MB" + (f" (+ {C * 7 * 8} bytes per get_results)" if n != "host" else ""))
        print(f"   host / device: {statistics.median(t['host']) / statistics.median(t['device']):.1f} x    "
              f"eager / device: {statistics.median(t['eager']) / statistics.median(t['device']):.1f} x")
        tr = seg_metrics.SegMetricsTracker(C)
        tr.update(logits, targets)
        show(f"SegMetricsTracker.update, logits {shape} bf16", *launches(lambda: tr.update(logits, targets)), top=6)
        show(f"eager composition, logits {shape} bf16",
             *launches(lambda: seg_metrics._eager_accumulate(tr.state, seg_metrics._eager_counts(logits, targets, C, False), H * W)), top=6)


if __name__ == "__main__":
    main()
