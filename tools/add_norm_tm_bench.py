"""vivim_amd.layernorm.add_layer_norm_tm (csrc/token_layernorm.hip) against the ATen composition it replaces in one warmed process,
on the rows the SegFormer blocks of the bench workload add and normalise (batch 3 x 5 frames at 256 x 256): (61440, 64),
(15360, 128), (3840, 320), (960, 512), with a bf16 branch on an fp32 residual (the autocast step) and all fp32.
    python tools/add_norm_tm_bench.py [--reps 200] [--rounds 7] [--no-step] [--steps 10]
The composition is `branch * mask + res` (DropPath's per-sample mask), F.layer_norm of the sum, and the cast the norm's consumer
(a Linear under autocast) adds.  One call is forward + backward: res, branch, weight and bias all require a gradient, and both
outputs (the sum and the norm) receive one; timed with device events around `reps` calls; the two implementations alternate,
round by round, and the table gives the median round with the fastest and the slowest beside it.  The yardstick is the composition
in the same run; under each pair, the GPU time of the kernels of one call (torch profiler).  Then (unless --no-step) the whole train
step: frames/s with build_model(fused_backbone_add_norm=False) and (True), in alternating windows of `steps` steps, and the kernel
launches of one step each way (tools/launch_count.py's counter)."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from layernorm_tm_bench import SHAPES, short  # noqa: E402
from upsample_bench import alternate  # noqa: E402

BRANCH_DTYPES = (torch.bfloat16, torch.float32)
SAMPLES = 15                                             # batch 3 x 5 frames


def bench_shape(rows, C, branch_dtype, reps, rounds):
    from vivim_amd import layernorm as ln
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    n = rows // SAMPLES
    res = torch.randn(SAMPLES, n, C, generator=g).to(dev).requires_grad_(True)
    branch = torch.randn(SAMPLES, n, C, generator=g).to(branch_dtype).to(dev).requires_grad_(True)
    w = (torch.randn(C, generator=g) * 0.5 + 1.0).to(dev).requires_grad_(True)
    b = (torch.randn(C, generator=g) * 0.3).to(dev).requires_grad_(True)
    scale = (torch.rand(SAMPLES, generator=g) < 0.8).float().div(0.8).to(dev)
    mask = scale.to(branch_dtype).view(SAMPLES, 1, 1)
    g_res = torch.randn(SAMPLES, n, C, generator=g).to(dev)
    g_y = torch.randn(SAMPLES, n, C, generator=g).to(dev).to(branch_dtype)
    assert ln.tm_add_supported(res, branch, w, b)

    def composition():
        h = branch * mask + res
        return h, F.layer_norm(h, (C,), w, b, 1e-5).to(branch_dtype)
    ops = {"ours": lambda: ln.add_layer_norm_tm(res, branch, w, b, 1e-5, scale=scale), "aten": composition}
    outs = {}
    for k, op in ops.items():
        h, y = op()
        outs[k] = (h.detach().float(), y.detach().float()) + tuple(t.float() for t in torch.autograd.grad((h, y), (res, branch, w, b),
                                                                                                         (g_res, g_y)))
    diff = [float((a - c).abs().max()) for a, c in zip(outs["ours"], outs["aten"])]

    def both(op):
        def run():
            torch.autograd.grad(op(), (res, branch, w, b), (g_res, g_y))
        return run
    res_ = alternate({k: both(op) for k, op in ops.items()}, reps, rounds)
    bsz = branch.element_size()
    nbytes = rows * C * (4 + bsz + 4 + bsz) + rows * C * (4 + bsz + 4 + 4 + bsz)   # fwd branch, res, res_new, y; bwd res_new, dy, dres, dres_in, dbranch
    name = f"({rows}, {C}) {str(branch_dtype).replace('torch.', '')} branch + float32 residual"
    print(f"{name}: {nbytes / 1e6:.1f} MB forward + backward; max|ours - aten| sum {diff[0]:.3e}, y {diff[1]:.3e}, dres {diff[2]:.3e}, "
          f"dbranch {diff[3]:.3e}, dweight {diff[4]:.3e}, dbias {diff[5]:.3e}")
    med = {k: statistics.median(v) for k, v in res_.items()}
    for k, v in res_.items():
        print(f"    fwd+bwd {k:5s} {med[k]:9.1f} us  (min {min(v):.1f}, max {max(v):.1f})  {nbytes / med[k] / 1e3:8.1f} GB/s")
    print(f"    fwd+bwd ours / aten = {med['ours'] / med['aten']:.2f}")
    from launch_count import launches
    for k, op in ops.items():
        names, dur = launches(both(op))
        print(f"    kernels {k:5s} {sum(dur.values()):9.1f} us in {sum(names.values())} launches: "
              + ", ".join(f"{dur[n]:.1f} {short(n)}" for n in sorted(dur, key=dur.get, reverse=True)))


def bench_step(steps, rounds):
    """off: the default model; on: fused_backbone_add_norm=True as shipped (layernorm.tm_add_worthwhile decides per site)."""
    from launch_count import launches
    from vivim_amd import train_step as ts
    dev = torch.device("cuda:0")
    models = {}
    for v, fused in (("off", False), ("on", True)):
        torch.manual_seed(0)
        model = ts.build_model(3, dev, fused_backbone_add_norm=fused)
        models[v] = (model, ts.make_optimizer(model))
    clip, onehot = ts.synthetic_batch(3, 5, 256, 3, dev, 0)
    frames = clip.shape[0] * clip.shape[1]

    def step(v):
        ts.train_step(*models[v], clip, onehot, 3, torch.bfloat16)
    for v in models:
        for _ in range(5):
            step(v)
    torch.cuda.synchronize()
    fps = {v: [] for v in models}
    for _ in range(rounds):
        for v in models:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(v)
            torch.cuda.synchronize()
            fps[v].append(steps * frames / (time.perf_counter() - t0))
    for v, f in fps.items():
        print(f"train step, fused_backbone_add_norm {v}: {statistics.median(f):.1f} frames/s  (min {min(f):.1f}, max {max(f):.1f}; "
              f"{rounds} windows of {steps} steps, batch 3 x 5 frames x 256 x 256, bf16)")
    for v in models:
        names, dur = launches(lambda: step(v))
        ours = {n: c for n, c in names.items() if "tln_" in n}
        elem = {n: c for n, c in names.items() if any(s in n for s in ("elementwise", "layer_norm", "LayerNorm", "GammaBeta", "tln_"))}
        print(f"train step, fused_backbone_add_norm {v}: {sum(names.values())} launches, {sum(dur.values()) / 1e3:.2f} ms of GPU time; "
              f"elementwise + LayerNorm kernels: {sum(elem.values())} launches, {sum(dur[n] for n in elem) / 1e3:.3f} ms; of them tln_*: "
              f"{sum(ours.values())} launches, {sum(dur[n] for n in ours) / 1e3:.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("add_norm_tm_bench.py measures on the GPU: none found")
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {a.reps} calls per round, {a.rounds} rounds")
    for branch_dtype in BRANCH_DTYPES:
        for rows, C in SHAPES:
            bench_shape(rows, C, branch_dtype, a.reps, a.rounds)
    if not a.no_step:
        bench_step(a.steps, a.rounds)


if __name__ == "__main__":
    main()
