"""vivim_amd.optimizer.FusedStepAdamW (csrc/optimizer.hip) against the optimizer phase of train_step it replaces, in one warmed
process on the bench model's real parameter list (build_model(3)) with seeded random gradients.
    python tools/optimizer_bench.py [--phases 50] [--rounds 7] [--steps 10] [--no-step] [--out profiles/r11_fused_optimizer.txt]
A phase is everything train_step does between backward() and its return: for fp16 the unscale, the overflow check with its host
synchronisation, clip_grad_norm_, LeanFusedAdamW.step and the scale policy; for bf16 the clip and the step.  The stock phase is
restated here from train_step.py and the fused one is FusedStepAdamW.step.  The two alternate round by round; a round is `phases`
phases ending in one synchronise, timed with device events (GPU) and a host clock (wall); the table gives the median round with
the fastest and the slowest beside it.  The yardstick is the stock sequence in the same run.  The loss scale is pinned to 1 on
both sides, so that the stock side's in-place unscale leaves the gradients as they are from phase to phase; its launches are the
same.  Then the kernels of one phase each way (torch profiler), the three kernels' bytes over their time against the HBM rate a
streaming kernel reaches on this part (6.3 TB/s), and -- unless --no-step -- the launches of one whole train step (fp16 and bf16,
clip 1.0) and its frames/s for fp16 + clip with the switch off and on, in alternating windows of `steps` steps."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_ACHIEVABLE = 6.3e12                                  # bytes/s, a float4 copy on this part
CASES = (("fp16 + clip 1.0", True, 1.0), ("bf16 + clip 1.0", False, 1.0), ("bf16, no clipping", False, None))
_out = []


def say(line=""):
    print(line, flush=True)
    _out.append(line)


def stock_phase(params, opt, sc, fp16, clip):
    """train_step.py's optimizer phase for a LeanFusedAdamW, gradients already in place."""
    if fp16:
        torch._foreach_mul_([p.grad for p in params], 1.0 / sc["scale"])
        finite = bool(torch.stack([torch.isfinite(p.grad).all() for p in params]).all())
        if finite:
            if clip is not None:
                torch.nn.utils.clip_grad_norm_(params, clip)
            opt.step()
            sc["good"] += 1
        else:
            sc["scale"], sc["good"] = sc["scale"] * 0.5, 0
        return
    if clip is not None:
        torch.nn.utils.clip_grad_norm_(params, clip)
    opt.step()


def timed_round(fn, phases):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(phases):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / phases, (time.perf_counter() - t0) * 1e6 / phases          # us per phase: GPU, wall


def bench_phases(model, phases, rounds):
    from launch_count import launches
    from vivim_amd import optimizer as O
    from vivim_amd import train_step as ts
    params = [p for p in model.parameters() if p.requires_grad]
    gen = torch.Generator().manual_seed(0)
    for p in params:
        p.grad = (1e-3 * torch.randn(p.shape, generator=gen)).to(p.device)
    stock = ts.make_optimizer(model)
    fused = ts.make_optimizer(model, fused_step=True)
    assert type(stock) is ts.LeanFusedAdamW and type(fused) is O.FusedStepAdamW
    fused.record.view(torch.float32)[O.SCALE] = 1.0
    numel = sum(p.numel() for p in params)
    say(f"parameters: {len(params)} tensors, {numel / 1e6:.2f} M elements; {fused.total_blocks} map rows of {O._lib.OPT_CHUNK} elements; "
        f"{len(fused._cuts)} kernel-argument tables of at most {O._lib.OPT_MAX_TENSORS}; {fused.launches_per_step} launches per fused step "
        f"({len(fused._cuts) + 1} without clipping and scaling)")
    for title, fp16, clip in CASES:
        sc = {"scale": 1.0, "good": 0}
        fns = {"stock": lambda: stock_phase(params, stock, sc, fp16, clip),
               "fused": lambda: fused.step(max_norm=clip, scaled=fp16)}
        for fn in fns.values():
            for _ in range(5):
                fn()
        res = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                res[k].append(timed_round(fn, phases))
        say(f"-- {title}: {phases} phases per round, {rounds} rounds, median (min, max) per phase")
        med = {}
        for k, v in res.items():
            gpu, wall = [x[0] for x in v], [x[1] for x in v]
            med[k] = (statistics.median(gpu), statistics.median(wall))
            say(f"   {k:5s} device events {med[k][0]:9.1f} us ({min(gpu):.1f}, {max(gpu):.1f})   wall {med[k][1]:9.1f} us "
                f"({min(wall):.1f}, {max(wall):.1f})")
        say(f"   fused / stock: device events {med['fused'][0] / med['stock'][0]:.2f}, wall {med['fused'][1] / med['stock'][1]:.2f}")
        for k, fn in fns.items():
            names, dur = launches(fn, warm=1)
            say(f"   kernels {k:5s} {sum(names.values()):5d} launches, {sum(dur.values()):9.1f} us of GPU time")
            if k == "fused":
                for n in sorted(dur, key=dur.get, reverse=True):
                    which = "stats" if "grad_stats" in n else "adamw" if "adamw" in n else "finalise" if "finalise" in n else None
                    nbytes = {"stats": 4 * numel + 8 * fused.total_blocks, "adamw": 28 * numel, "finalise": 8 * fused.total_blocks + 64,
                              None: 0}[which]
                    rate = nbytes / (dur[n] * 1e-6) if dur[n] else 0.0
                    say(f"      {names[n]:3d} x {n[:60]:60s} {dur[n]:9.1f} us  {nbytes / 1e6:9.2f} MB  {rate / 1e12:5.2f} TB/s = "
                        f"{100 * rate / HBM_ACHIEVABLE:5.1f} % of {HBM_ACHIEVABLE / 1e12:.1f} TB/s")
    for p in params:
        p.grad = None


def bench_step(model, steps, rounds):
    from launch_count import launches
    from vivim_amd import train_step as ts
    dev = next(model.parameters()).device
    opts = {"off": ts.make_optimizer(model), "on": ts.make_optimizer(model, fused_step=True)}
    clip, onehot = ts.synthetic_batch(3, 5, 256, 3, dev, 0)
    frames = clip.shape[0] * clip.shape[1]
    for amp, name in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        for v, opt in opts.items():
            names, dur = launches(lambda: ts.train_step(model, opt, clip, onehot, 3, amp, clip_grad_norm=1.0))
            ours = {n: c for n, c in names.items() if "opt_" in n}
            say(f"train step, {name} + clip 1.0, fused_step {v}: {sum(names.values())} launches, {sum(dur.values()) / 1e3:.2f} ms of GPU "
                f"time; of them opt_*: {sum(ours.values())} launches, {sum(dur[n] for n in ours) / 1e3:.3f} ms")
    fps = {v: [] for v in opts}
    for _ in range(rounds):
        for v, opt in opts.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                ts.train_step(model, opt, clip, onehot, 3, torch.float16, clip_grad_norm=1.0)
            torch.cuda.synchronize()
            fps[v].append(steps * frames / (time.perf_counter() - t0))
    for v, f in fps.items():
        say(f"train step, fp16 + clip 1.0, fused_step {v}: {statistics.median(f):.1f} frames/s  (min {min(f):.1f}, max {max(f):.1f}; "
            f"{rounds} windows of {steps} steps, batch 3 x 5 frames x 256 x 256)")
    say(f"   on / off = {statistics.median(fps['on']) / statistics.median(fps['off']):.3f}; loss scale after the run: off "
        f"{ts._SCALERS[id(opts['off'])]['scale']:g}, on {float(opts['on'].loss_scale):g}; skipped steps on: {int(opts['on'].skipped_steps)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phases", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "r11_fused_optimizer.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optimizer_bench.py measures on the GPU: none found")
    from vivim_amd import train_step as ts
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    torch.manual_seed(0)
    bench_phases(ts.build_model(3, torch.device("cuda:0")), a.phases, a.rounds)
    if not a.no_step:
        torch.manual_seed(0)                             # a fresh model: the phases above moved the first one's parameters
        bench_step(ts.build_model(3, torch.device("cuda:0")), a.steps, a.rounds)
    with open(a.out, "w") as f:
        f.write("\n".join(_out) + "\n")


if __name__ == "__main__":
    main()
