"""vivim_amd.bilinear_upsample (csrc/upsample.hip) against ATen's F.interpolate in one warmed process, on the shapes of the
bench workload (batch 3 x 5 frames at 256 x 256): the three decode-head features that really upsample, (15, 768, s, s) -> 64 x 64
for s = 8, 16, 32 in channels-last bf16 (and fp32: what the step under autocast passes), and the logits, (15, 3, 64, 64) -> 256 x 256 in planes bf16 and fp32.
    python tools/upsample_bench.py [--reps 200] [--rounds 7] [--no-step] [--steps 10]
Forward and backward are timed separately with device events around `reps` launches; the two implementations alternate, round
by round, and the table gives the median round with the fastest and the slowest beside it.  The yardstick is ATen in the same
run.  Then (unless --no-step) the whole train step, frames/s with Vivim(fused_upsample=False) and (True) in alternating windows
of `steps` steps, and the kernel launches of one step either way (tools/launch_count.py's counter)."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPES = [((15, 768, s, s), (64, 64), "cl", dt) for dt in (torch.bfloat16, torch.float32) for s in (8, 16, 32)] + \
         [((15, 3, 64, 64), (256, 256), "planes", dt) for dt in (torch.bfloat16, torch.float32)]


def timed(fn, reps):
    """Microseconds per call of `reps` back-to-back calls, by device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def alternate(fns, reps, rounds):
    """{name: [us per call, one per round]} with the implementations taking turns inside every round."""
    for fn in fns.values():                                  # warm-up: code objects, allocator blocks
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, reps))
    return out


def bench_shape(shape, size, layout, dtype, reps, rounds):
    from vivim_amd import bilinear_upsample, upsample
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    fmt = torch.channels_last if layout == "cl" else torch.contiguous_format
    x = torch.randn(*shape, generator=g).to(dev).to(dtype).contiguous(memory_format=fmt).requires_grad_(True)
    go = torch.randn(shape[0], shape[1], *size, generator=g).to(dev).to(dtype).contiguous(memory_format=fmt)
    assert upsample.supported(x, size)
    ops = {"ours": lambda t: bilinear_upsample(t, size),
           "aten": lambda t: F.interpolate(t, size=size, mode="bilinear", align_corners=False)}
    ys = {k: op(x) for k, op in ops.items()}
    gx = {k: torch.autograd.grad(ys[k], x, go, retain_graph=True)[0] for k in ops}
    dy = (ys["ours"].detach().float() - ys["aten"].detach().float()).abs().max()
    ddx = (gx["ours"].float() - gx["aten"].float()).abs().max()

    def fwd(op):
        def run():
            with torch.no_grad():
                op(x)
        return run
    res = alternate({f"{k} fwd": fwd(op) for k, op in ops.items()}, reps, rounds)
    res.update(alternate({f"{k} bwd": (lambda k=k: torch.autograd.grad(ys[k], x, go, retain_graph=True)) for k in ops},
                         reps, rounds))
    nbytes = (x.numel() + go.numel()) * x.element_size()
    name = f"{tuple(shape)} -> {size} {layout} {str(dtype).replace('torch.', '')}"
    print(f"{name}: {nbytes / 1e6:.1f} MB either way; max|ours - aten| forward {float(dy):.3e}, backward {float(ddx):.3e}")
    for d in ("fwd", "bwd"):
        med = {k: statistics.median(res[f"{k} {d}"]) for k in ops}
        for k in ops:
            v = res[f"{k} {d}"]
            print(f"    {d} {k:5s} {med[k]:9.1f} us  (min {min(v):.1f}, max {max(v):.1f})  {nbytes / med[k] / 1e3:8.1f} GB/s")
        print(f"    {d} ours / aten = {med['ours'] / med['aten']:.2f}")


def bench_step(steps, rounds):
    from launch_count import launches
    from vivim_amd import train_step as ts
    dev = torch.device("cuda:0")
    models = {}
    for fused in (False, True):
        torch.manual_seed(0)
        model = ts.build_model(3, dev, fused_upsample=fused)
        models[fused] = (model, ts.make_optimizer(model))
    clip, onehot = ts.synthetic_batch(3, 5, 256, 3, dev, 0)
    frames = clip.shape[0] * clip.shape[1]

    def step(fused):
        model, opt = models[fused]
        ts.train_step(model, opt, clip, onehot, 3, torch.bfloat16)
    for fused in models:
        for _ in range(5):
            step(fused)
    torch.cuda.synchronize()
    fps = {False: [], True: []}
    for _ in range(rounds):
        for fused in models:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(fused)
            torch.cuda.synchronize()
            fps[fused].append(steps * frames / (time.perf_counter() - t0))
    for fused in models:
        v = fps[fused]
        print(f"train step, fused_upsample={fused}: {statistics.median(v):.1f} frames/s  (min {min(v):.1f}, max {max(v):.1f}; "
              f"{rounds} windows of {steps} steps, batch 3 x 5 frames x 256 x 256, bf16)")
    for fused in models:
        names, dur = launches(lambda: step(fused))
        ups = {n: c for n, c in names.items() if "upsample" in n.lower()}
        print(f"train step, fused_upsample={fused}: {sum(names.values())} launches, {sum(dur.values()) / 1e3:.2f} ms of GPU time; "
              f"upsampling kernels:")
        for n, c in sorted(ups.items()):
            print(f"    {c:4d} {dur[n] / 1e3:8.3f} ms  {n}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("upsample_bench.py measures on the GPU: none found")
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {a.reps} launches per round, {a.rounds} rounds")
    for shape, size, layout, dtype in SHAPES:
        bench_shape(shape, size, layout, dtype, a.reps, a.rounds)
    if not a.no_step:
        bench_step(a.steps, a.rounds)


if __name__ == "__main__":
    main()
