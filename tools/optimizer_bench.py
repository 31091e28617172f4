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
clip 1.0) and its frames/s for fp16 + clip with the switch off and on, in alternating windows of `steps` steps.
    python tools/optimizer_bench.py --master-weights [--out profiles/r12_master_weights.txt]
measures master weights instead (lower_params + FusedStepAdamW(master_weights=True)): the yardstick is the fp32 fused step of the
same run.  The phase of the lowered parameter list (bf16 and fp16) against the fp32 one, round by round, with opt_adamw's time and
bytes per second in both forms; then the whole train step with the parameters stock and lowered, both under fused_step=True:
launches, GPU time, the cast kernels by name, frames/s in alternating windows and the allocator's peak over a step."""
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


def _cast_kernels(names):
    """Launches of torch's dtype-converting copy kernels, by the conversion their name states."""
    out = {}
    for n, c in names.items():
        key = next((k for k in ("bfloat16tofloat32", "float16tofloat32", "halftofloat32", "bfloat16_copy", "float16_copy", "half_copy")
                    if k in n.lower()), None)
        if key:
            out[key] = out.get(key, 0) + c
    return out


def bench_master_weights(phases, rounds, steps):
    from launch_count import launches
    from vivim_amd import optimizer as O
    from vivim_amd import train_step as ts
    dev = torch.device("cuda:0")
    clip, onehot = ts.synthetic_batch(3, 5, 256, 3, dev, 0)
    frames = clip.shape[0] * clip.shape[1]
    for amp, name in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
        torch.manual_seed(0)
        models = {"off": ts.build_model(3, dev)}
        torch.manual_seed(0)
        models["on"] = ts.build_model(3, dev, low_precision_params=amp)
        opts = {"off": ts.make_optimizer(models["off"], fused_step=True),
                "on": ts.make_optimizer(models["on"], fused_step=True, master_weights=True)}
        on = opts["on"]
        n_low = sum(w is not None for w in on.masters)
        low_numel = sum(p.numel() for p, w in zip(on.params, on.masters) if w is not None)
        numel = sum(p.numel() for p in on.params)
        say(f"== {name}: {n_low} of {len(on.params)} trained tensors lowered ({low_numel / 1e6:.2f} of {numel / 1e6:.2f} M elements); "
            f"launches per step: fp32 {opts['off'].launches_per_step} ({len(opts['off']._cuts)} tables), master weights "
            f"{on.launches_per_step} ({len(on._cuts)} tables)")
        # ---- the optimizer phase alone, seeded gradients in each parameter's dtype
        gen = torch.Generator().manual_seed(0)
        for p_off, p_on in zip(opts["off"].params, on.params):
            g = 1e-3 * torch.randn(p_off.shape, generator=gen)
            p_off.grad, p_on.grad = g.to(dev), g.to(dev, p_on.dtype)
        for o in opts.values():
            o.record.view(torch.float32)[O.SCALE] = 1.0
        scaled = amp == torch.float16
        fns = {"fp32": lambda: opts["off"].step(max_norm=1.0, scaled=scaled), "master": lambda: on.step(max_norm=1.0, scaled=scaled)}
        for fn in fns.values():
            for _ in range(5):
                fn()
        res = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                res[k].append(timed_round(fn, phases))
        say(f"-- optimizer phase, {name} + clip 1.0: {phases} phases per round, {rounds} rounds, median (min, max) per phase")
        med = {}
        for k, v in res.items():
            gpu, wall = [x[0] for x in v], [x[1] for x in v]
            med[k] = (statistics.median(gpu), statistics.median(wall))
            say(f"   {k:6s} device events {med[k][0]:9.1f} us ({min(gpu):.1f}, {max(gpu):.1f})   wall {med[k][1]:9.1f} us "
                f"({min(wall):.1f}, {max(wall):.1f})")
        say(f"   master / fp32: device events {med['master'][0] / med['fp32'][0]:.3f}, wall {med['master'][1] / med['fp32'][1]:.3f}")
        adamw = {}
        for k, fn in fns.items():
            names, dur = launches(fn, warm=1)
            say(f"   kernels {k:6s} {sum(names.values()):5d} launches, {sum(dur.values()):9.1f} us of GPU time")
            for n in sorted(dur, key=dur.get, reverse=True):
                say(f"      {names[n]:3d} x {n[:70]:70s} {dur[n]:9.1f} us")
            adamw[k] = sum(d for n, d in dur.items() if "opt_adamw" in n)
        for k in fns:                                       # 28 bytes per element in either form
            rate = 28 * numel / (adamw[k] * 1e-6)
            say(f"   opt_adamw, {k:6s}: {adamw[k]:8.1f} us for {28 * numel / 1e6:.2f} MB = {rate / 1e12:.2f} TB/s = "
                f"{100 * rate / HBM_ACHIEVABLE:.1f} % of {HBM_ACHIEVABLE / 1e12:.1f} TB/s")
        say(f"   opt_adamw master / fp32 = {adamw['master'] / adamw['fp32']:.3f}")
        for o in opts.values():
            o.zero_grad()
        # ---- the whole train step
        def step(v):
            return ts.train_step(models[v], opts[v], clip, onehot, 3, amp, clip_grad_norm=1.0)
        counts = {}
        for v in opts:
            names, dur = launches(lambda: step(v))
            counts[v] = sum(names.values())
            ours = {n: c for n, c in names.items() if "opt_" in n}
            say(f"train step, {name} + clip 1.0, fused_step on, master weights {v}: {counts[v]} launches, {sum(dur.values()) / 1e3:.2f} ms "
                f"of GPU time; opt_*: {sum(ours.values())} launches, {sum(dur[n] for n in ours) / 1e3:.3f} ms; cast kernels: {_cast_kernels(names)}")
        say(f"   launches off - on = {counts['off'] - counts['on']}; lowered tensors: {n_low} (two casts each: {2 * n_low}), extra optimizer "
            f"launches: {on.launches_per_step - opts['off'].launches_per_step}")
        fps, peak = {v: [] for v in opts}, {}
        for _ in range(rounds):
            for v in opts:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    step(v)
                torch.cuda.synchronize()
                fps[v].append(steps * frames / (time.perf_counter() - t0))
        for v, f in fps.items():
            say(f"train step, {name} + clip 1.0, master weights {v}: {statistics.median(f):.1f} frames/s  (min {min(f):.1f}, max {max(f):.1f}; "
                f"{rounds} windows of {steps} steps, batch 3 x 5 frames x 256 x 256)")
        say(f"   on / off = {statistics.median(fps['on']) / statistics.median(fps['off']):.3f}")
        for v in opts:
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step(v)
            torch.cuda.synchronize()
            peak[v] = torch.cuda.max_memory_allocated()
            say(f"allocator, {name}, master weights {v}: {base / 2**20:.0f} MiB before the step (both models resident), peak "
                f"{peak[v] / 2**20:.0f} MiB, the step's own {(peak[v] - base) / 2**20:.0f} MiB")
        del models, opts, on, fns
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phases", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--master-weights", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optimizer_bench.py measures on the GPU: none found")
    from vivim_amd import train_step as ts
    a.out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                  "r12_master_weights.txt" if a.master_weights else "r11_fused_optimizer.txt")
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    if a.master_weights:
        bench_master_weights(a.phases, a.rounds, a.steps)
        with open(a.out, "w") as f:
            f.write("\n".join(_out) + "\n")
        return
    torch.manual_seed(0)
    bench_phases(ts.build_model(3, torch.device("cuda:0")), a.phases, a.rounds)
    if not a.no_step:
        torch.manual_seed(0)                             # a fresh model: the phases above moved the first one's parameters
        bench_step(ts.build_model(3, torch.device("cuda:0")), a.steps, a.rounds)
    with open(a.out, "w") as f:
        f.write("\n".join(_out) + "\n")


if __name__ == "__main__":
    main()
