"""vivim_amd.layernorm.layer_norm_tm (csrc/token_layernorm.hip) against ATen's F.layer_norm in one warmed process, on the rows
the SegFormer blocks of the bench workload normalise (batch 3 x 5 frames at 256 x 256): (61440, 64), (15360, 128), (3840, 320),
(960, 512), with an fp32 input and a bf16 output (the autocast step with the switch on; ATen writes fp32 there and its consumer
casts: the cast kernel is timed with ATen's side) and fp32 / fp32.
    python tools/layernorm_tm_bench.py [--reps 200] [--rounds 7] [--no-step] [--steps 10]
One call is forward + backward (x, weight and bias all require a gradient), timed with device events around `reps` calls; the
two implementations alternate, round by round, and the table gives the median round with the fastest and the slowest beside it.
The yardstick is ATen in the same run; under each pair, the GPU time of the kernels of one call (torch profiler).  Then (unless --no-step) the whole train step: frames/s with
build_model(fast_backbone_layernorm=False), with (True) as shipped and with (True) and tm_worthwhile forced to "always", in
alternating windows of `steps` steps, and the kernel launches of one step each way (tools/launch_count.py's counter)."""
import argparse
import os
import re
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from upsample_bench import alternate  # noqa: E402

SHAPES = [(61440, 64), (15360, 128), (3840, 320), (960, 512)]
OUT_DTYPES = (torch.bfloat16, torch.float32)


def short(name):
    """A kernel's own name out of its (possibly mangled) signature."""
    m = re.search(r"\d+(tln_\w+?_kernel)", name) if name.startswith("_Z") else None
    if m:
        return m.group(1)
    return re.split(r"[<(]", name.replace("(anonymous namespace)::", "").replace("void ", ""))[0].split("::")[-1]


def bench_shape(rows, C, out_dtype, reps, rounds):
    from vivim_amd import layernorm as ln
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(rows, C, generator=g).to(dev).requires_grad_(True)
    w = (torch.randn(C, generator=g) * 0.5 + 1.0).to(dev).requires_grad_(True)
    b = (torch.randn(C, generator=g) * 0.3).to(dev).requires_grad_(True)
    go = torch.randn(rows, C, generator=g).to(dev).to(out_dtype)
    assert ln.tm_supported(x, w, b)
    # ATen's side of the bf16 case: layer_norm in fp32 and the cast its consumer (a Linear under autocast) adds
    ops = {"ours": lambda: ln.layer_norm_tm(x, w, b, 1e-5, out_dtype=out_dtype),
           "aten": lambda: F.layer_norm(x, (C,), w, b, 1e-5).to(out_dtype)}
    outs = {}
    for k, op in ops.items():
        y = op()
        outs[k] = (y.detach().float(),) + tuple(t.float() for t in torch.autograd.grad(y, (x, w, b), go))
    diff = [float((a - c).abs().max()) for a, c in zip(outs["ours"], outs["aten"])]

    def both(op):
        def run():
            torch.autograd.grad(op(), (x, w, b), go)
        return run
    res = alternate({k: both(op) for k, op in ops.items()}, reps, rounds)
    osz = go.element_size()
    nbytes = rows * C * (4 + osz) + rows * C * (4 + osz + 4)        # forward x, y; backward x, dy, dx
    name = f"({rows}, {C}) float32 -> {str(out_dtype).replace('torch.', '')}"
    print(f"{name}: {nbytes / 1e6:.1f} MB forward + backward; max|ours - aten| y {diff[0]:.3e}, dx {diff[1]:.3e}, "
          f"dweight {diff[2]:.3e}, dbias {diff[3]:.3e}")
    med = {k: statistics.median(v) for k, v in res.items()}
    for k, v in res.items():
        print(f"    fwd+bwd {k:5s} {med[k]:9.1f} us  (min {min(v):.1f}, max {max(v):.1f})  {nbytes / med[k] / 1e3:8.1f} GB/s")
    print(f"    fwd+bwd ours / aten = {med['ours'] / med['aten']:.2f}")
    # a call is a handful of short kernels and its host side can be the longer part: the kernels' own time, from the profiler
    from launch_count import launches
    for k, op in ops.items():
        names, dur = launches(both(op))
        print(f"    kernels {k:5s} {sum(dur.values()):9.1f} us in {sum(names.values())} launches: "
              + ", ".join(f"{dur[n]:.1f} {short(n)}" for n in sorted(dur, key=dur.get, reverse=True)))


def bench_step(steps, rounds):
    """off: the default model; on: fast_backbone_layernorm=True as shipped (layernorm.tm_worthwhile decides per call); always: the
    same model with tm_worthwhile answering True everywhere."""
    from launch_count import launches
    from vivim_amd import layernorm as ln
    from vivim_amd import train_step as ts
    dev = torch.device("cuda:0")
    models = {}
    for fast in (False, True):
        torch.manual_seed(0)
        model = ts.build_model(3, dev, fast_backbone_layernorm=fast)
        models[fast] = (model, ts.make_optimizer(model))
    clip, onehot = ts.synthetic_batch(3, 5, 256, 3, dev, 0)
    frames = clip.shape[0] * clip.shape[1]
    shipped = ln.tm_worthwhile

    def step(variant):
        model, opt = models[variant != "off"]
        ln.tm_worthwhile = (lambda x: True) if variant == "always" else shipped
        try:
            ts.train_step(model, opt, clip, onehot, 3, torch.bfloat16)
        finally:
            ln.tm_worthwhile = shipped
    variants = ("off", "on", "always")
    for v in variants:
        for _ in range(5):
            step(v)
    torch.cuda.synchronize()
    fps = {v: [] for v in variants}
    for _ in range(rounds):
        for v in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(v)
            torch.cuda.synchronize()
            fps[v].append(steps * frames / (time.perf_counter() - t0))
    for v in variants:
        f = fps[v]
        print(f"train step, fast_backbone_layernorm {v}: {statistics.median(f):.1f} frames/s  (min {min(f):.1f}, max {max(f):.1f}; "
              f"{rounds} windows of {steps} steps, batch 3 x 5 frames x 256 x 256, bf16)")
    for v in variants:
        names, dur = launches(lambda: step(v))
        norm = {n: c for n, c in names.items()
                if any(s in n for s in ("layer_norm", "LayerNorm", "GammaBeta", "tln_", "ln_cm", "ln_reduce"))}
        casts = {n: c for n, c in names.items() if "copy" in n.lower()}
        print(f"train step, fast_backbone_layernorm {v}: {sum(names.values())} launches, {sum(dur.values()) / 1e3:.2f} ms of GPU time; "
              f"copy / cast kernels: {sum(casts.values())} launches, {sum(dur[n] for n in casts) / 1e3:.3f} ms; LayerNorm kernels: "
              f"{sum(norm.values())} launches, {sum(dur[n] for n in norm) / 1e3:.3f} ms")
        for n, c in sorted(norm.items()):
            print(f"    {c:4d} {dur[n] / 1e3:8.3f} ms  {short(n)}  {n[:60]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("layernorm_tm_bench.py measures on the GPU: none found")
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {a.reps} calls per round, {a.rounds} rounds")
    for out_dtype in OUT_DTYPES:
        for rows, C in SHAPES:
            bench_shape(rows, C, out_dtype, a.reps, a.rounds)
    if not a.no_step:
        bench_step(a.steps, a.rounds)


if __name__ == "__main__":
    main()
