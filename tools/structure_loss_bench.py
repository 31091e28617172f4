"""The structure loss, eager composition (structure_loss.multiclass_structure_loss / structure_loss) against the fused kernels
(csrc/structure_loss.hip): forward + backward time by device events with both routes alternating round by round in one warmed
process (the median of the rounds), kernel launches of one forward + backward (torch.profiler), and the allocator's peak above the
inputs.  The yardstick is the eager composition of the same run.
    python tools/structure_loss_bench.py [--iters 200] [--rounds 7]"""
import argparse
import collections
import os
import statistics
import sys

import torch
from torch.profiler import ProfilerActivity, profile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (N, C, H, W), dtype, binary: the bench workload (batch 3 x clip 5), 512^2 at batch 8 x clip 5, and the binary recipe in fp32
CASES = (((15, 3, 256, 256), torch.bfloat16, False), ((40, 3, 512, 512), torch.bfloat16, False), ((15, 1, 256, 256), torch.float32, True))


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


def launches(fn):
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    names = collections.Counter(ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
    return sum(names.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "structure_loss_bench needs a GPU"
    dev = torch.device("cuda:0")
    from vivim_amd import structure_loss as sl
    for shape, dtype, binary in CASES:
        N, C, H, W = shape
        g = torch.Generator().manual_seed(0)
        logits = (torch.randn(shape, generator=g) * 4).to(dtype).to(dev).requires_grad_(True)
        labels = torch.randint(0, 2 if binary else C, (N, H, W), generator=g)
        labels[:, : H // 2, : W // 3] = 1                    # a solid region next to the noise
        labels = labels.to(dev)
        if binary:
            mask = (labels == 1)[:, None]                    # bool: taken as it is, no host synchronisation
            fmask = mask.float()
            assert sl._binary_labels(logits, mask) is not None
            variants = (("eager", lambda: sl.structure_loss(logits, fmask)), ("fused", lambda: sl.structure_loss_fused(logits, mask)))
        else:
            assert sl.supported(logits, labels, C)
            variants = (("eager", lambda: sl.multiclass_structure_loss(logits, labels, C)),
                        ("fused", lambda: sl.multiclass_structure_loss_fused(logits, labels, C)))

        def call(fn):
            logits.grad = None
            fn().backward()
        for _, fn in variants:                               # warm both
            timed(lambda: call(fn), 10)
        times = {n: [] for n, _ in variants}
        for _ in range(a.rounds):                            # alternate round by round
            for n, fn in variants:
                times[n].append(timed(lambda: call(fn), a.iters))
        count = {n: launches(lambda: call(fn)) for n, fn in variants}
        mem = {n: peak_bytes(lambda: call(fn)) for n, fn in variants}
        values = {n: float(fn().detach()) for n, fn in variants}
        print(f"== structure loss forward + backward, logits {shape} {str(dtype).replace('torch.', '')}, "
              f"{'bool mask' if binary else 'int64 targets'}, {a.iters} calls x {a.rounds} rounds (device events)")
        for n, _ in variants:
            t = times[n]
            print(f"   {n:6s} median {statistics.median(t) * 1e3:9.1f} us  min {min(t) * 1e3:9.1f}  max {max(t) * 1e3:9.1f}   "
                  f"{count[n]:4d} launches   peak memory above the inputs {mem[n] / 2 ** 20:9.1f} MiB")
        print(f"   eager / fused {statistics.median(times['eager']) / statistics.median(times['fused']):.2f}x   "
              f"loss eager {values['eager']:.7f} fused {values['fused']:.7f}")


if __name__ == "__main__":
    main()
