"""The recall-focused loss, eager chain (train_step.recall_focused_loss) against the fused kernels (seg_loss.py): forward + backward
time by device events with both variants alternating in one warmed process, peak memory of one forward + backward, and the train
step's frames/s with fused_loss off and on.
    python tools/seg_loss_bench.py [--iters 200] [--rounds 5] [--steps 30] [--no-step]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((15, 3, 256, 256), (40, 3, 512, 512))          # the bench workload (batch 3 x clip 5); 512^2, batch 8 x clip 5


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters                   # ms per call


def peak_bytes(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "seg_loss_bench needs a GPU"
    dev = torch.device("cuda:0")
    from vivim_amd import train_step as ts
    from vivim_amd.seg_loss import recall_focused_loss_fused, supported
    variants = (("eager", ts.recall_focused_loss), ("fused", recall_focused_loss_fused))
    for shape in SHAPES:
        N, C, H, W = shape
        g = torch.Generator().manual_seed(0)
        logits = (torch.randn(shape, generator=g) * 4).to(torch.bfloat16).to(dev).requires_grad_(True)
        target = torch.randint(0, C, (N, H, W), generator=g).to(dev)
        assert supported(logits, target, C, 2.0)
        iters = a.iters if N * H * W < 4e6 else max(a.iters // 4, 10)

        def call(fn):
            logits.grad = None
            fn(logits, target, C).backward()
        for _, fn in variants:                               # warm both
            timed(lambda: call(fn), 10)
        times = {n: [] for n, _ in variants}
        for _ in range(a.rounds):                            # alternate
            for n, fn in variants:
                times[n].append(timed(lambda: call(fn), iters))
        mem = {n: peak_bytes(lambda: call(fn)) for n, fn in variants}
        le = float(ts.recall_focused_loss(logits, target, C))
        lf = float(recall_focused_loss_fused(logits, target, C))
        print(f"== loss forward + backward, logits {shape} bf16, int64 targets, {iters} calls x {a.rounds} rounds (device events)")
        for n, _ in variants:
            t = times[n]
            print(f"   {n:6s} median {statistics.median(t) * 1e3:9.1f} us  min {min(t) * 1e3:9.1f}  max {max(t) * 1e3:9.1f}   "
                  f"peak memory above the inputs {mem[n] / 2 ** 20:9.1f} MiB")
        print(f"   loss eager {le:.7f} fused {lf:.7f}")
    if a.no_step:
        return
    model = ts.build_model(3, dev)
    opt = ts.make_optimizer(model)
    clip, onehot = ts.synthetic_batch(3, 5, 256, 3, dev, 0)
    frames = clip.shape[0] * clip.shape[1]

    def steps(fused, n):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            ts.train_step(model, opt, clip, onehot, 3, torch.bfloat16, fused_loss=fused)
        e1.record()
        e1.synchronize()
        return frames * n / (e0.elapsed_time(e1) * 1e-3)
    for fused in (False, True):
        steps(fused, 5)
    fps = {False: [], True: []}
    for _ in range(a.rounds):
        for fused in (False, True):
            fps[fused].append(steps(fused, a.steps))
    print(f"== train_step, batch 3 x clip 5 x 256^2 bf16, {a.steps} steps x {a.rounds} rounds alternating")
    for fused in (False, True):
        t = fps[fused]
        print(f"   fused_loss={fused!s:5s} median {statistics.median(t):7.2f} frames/s  min {min(t):7.2f}  max {max(t):7.2f}")


if __name__ == "__main__":
    main()
