"""The training decode head, stock against Vivim(fused_head_concat=True) (vivim_amd/head_concat.py, csrc/head_concat.hip), in one
warmed process.
    python tools/head_concat_bench.py [--reps 20] [--rounds 7] [--no-large] [--train-step] [--kernels-only]
`Vivim.decode` forward + backward in train mode on random encoder states at the bench workload's head, (15; 64^2, 32^2, 16^2, 8^2),
under bf16 autocast and in fp32, and at (40; 128^2, 64^2, 32^2, 16^2) under bf16 autocast: device events around `reps` calls, the
two routes alternating round by round, the median round with the fastest and the slowest beside it; the allocator's peak over one
forward + backward of either route; the two kernels alone by the events of the _lib profile hook, with their achieved bytes/s over
the bytes the algorithm needs (_lib.algorithmic_bytes).  At the large shape also,
in eval mode (no dropout, BatchNorm on its running statistics, so that one image can be recomputed alone): the last image's
logits of both routes against an fp64 head.
--train-step: the train step at the bench's size (clip of 3 x 5 frames at 256^2, bf16), switch off and on in alternating windows of
10 steps.  --kernels-only: a few calls of the new route at the first shape and nothing else, for a counters-free
`rocprofv3 --kernel-trace --stats -- python tools/head_concat_bench.py --kernels-only`.
The yardstick is the stock route of the same run."""
import argparse
import copy
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS = (64, 128, 320, 512)
SHAPES = [(15, 64, (torch.bfloat16, torch.float32)), (40, 128, (torch.bfloat16,))]   # frames, stage-0 edge (the other stages halve it)


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
    for fn in fns.values():                                  # warm-up: code objects, library heuristics, allocator blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, reps))
    return out


def report(label, v, unit="us"):
    print(f"    {label:34s} {statistics.median(v):10.1f} {unit}  (min {min(v):.1f}, max {max(v):.1f})")
    return statistics.median(v)


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def states_for(frames, edge, dev):
    g = torch.Generator().manual_seed(frames)
    return tuple(torch.randn(frames, c, edge >> s, edge >> s, generator=g).to(dev) for s, c in enumerate(DIMS))


def head_step(model, states, switch, amp):
    def run():
        model.fused_head_concat = switch
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=amp, enabled=amp != torch.float32):
            out = model.decode(states, 1, states[0].shape[0])
        out.float().square().mean().backward()
        return out
    return run


def kernels_alone(model, states, amp, calls):
    """{entry point: (median us, algorithmic bytes of the first call)} of the two kernels over `calls` forward + backward passes of
    the new route.  The coins differ from call to call, and with them the masks read: 47 MB per dropped-out map at the bench's
    shape, and a slower backward when a small map is dropped out (profiles/r14_head_concat.txt has the spread)."""
    from vivim_amd import _lib
    run = head_step(model, states, True, amp)
    run()
    _lib.profile_begin(all_kernels=True)
    for _ in range(calls):
        run()
    rec = [r for r in _lib.profile_end() if r[0].startswith("vivim_head_concat")]
    out = {}
    for name in ("vivim_head_concat_fwd", "vivim_head_concat_bwd"):
        rows = [r for r in rec if r[0] == name]
        out[name] = (statistics.median(r[2] for r in rows) * 1e6, rows[0][1])
    return out


def last_image_against_fp64(model, states, dev):
    """Eval mode, bf16 autocast: rel. error (norm-wise) of the last image's logits, stock and new, against an fp64 head run on that
    image alone."""
    model.eval()
    try:
        ref = copy.deepcopy(model).double()
        ref.fused_head_concat = False
        with torch.no_grad():
            want = ref.decode(tuple(s[-1:].double() for s in states), 1, 1)
        del ref
        got = {}
        for switch in (False, True):
            model.fused_head_concat = switch
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                got[switch] = model.decode(states, 1, states[0].shape[0])[-1:].double()
        return {k: float((v - want).norm() / want.norm()) for k, v in got.items()}
    finally:
        model.train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-large", action="store_true")
    ap.add_argument("--train-step", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_concat_bench.py measures on the GPU: none found")
    from vivim_amd import head_concat
    from vivim_amd import train_step as ts
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {a.reps} calls per round, {a.rounds} rounds")
    torch.manual_seed(0)
    model = ts.build_model(3, dev, fused_head_concat=True).train()
    if a.kernels_only:
        states = states_for(15, 64, dev)
        run = head_step(model, states, True, torch.bfloat16)
        for _ in range(10):
            run()
        torch.cuda.synchronize()
        print("10 forward + backward passes of the new route at (15; 64^2 ...) bf16 done")
        return
    for frames, edge, amps in SHAPES[:1] if a.no_large else SHAPES:
        states = states_for(frames, edge, dev)
        for amp in amps:
            name = f"({frames}; " + ", ".join(f"{edge >> s}^2" for s in range(4)) + f") {'bf16 autocast' if amp != torch.float32 else 'fp32'}"
            off, on = head_step(model, states, False, amp), head_step(model, states, True, amp)
            with torch.autocast("cuda", dtype=amp, enabled=amp != torch.float32):
                feats = [mlp(s).permute(0, 2, 1).reshape(frames, -1, s.shape[2], s.shape[3])
                         for s, mlp in zip(states, model._decoder_projections())]
                assert head_concat.supported(feats[::-1], states[0].shape[2:])
            del feats
            res = alternate({"stock": off, "new": on}, a.reps, a.rounds)
            print(f"{name}: Vivim.decode forward + backward, train mode")
            stock, new = report("switch off (stock)", res["stock"]), report("switch on (head_concat)", res["new"])
            print(f"    on / off = {new / stock:.3f}")
            print(f"    allocator peak over one forward + backward: off {peak_mib(off):.0f} MiB, on {peak_mib(on):.0f} MiB")
            for kname, (us, nbytes) in kernels_alone(model, states, amp, 20).items():
                print(f"    {kname:34s} {us:10.1f} us  {nbytes / 1e6:.1f} MB algorithmic: {nbytes / us / 1e3:.1f} GB/s")
        if edge == 128:
            rel = last_image_against_fp64(model, states, dev)
            print(f"    eval mode, bf16 autocast, last image's logits against an fp64 head: stock {rel[False]:.3e}, new {rel[True]:.3e}")
    if a.train_step:
        opt = ts.make_optimizer(model)
        clip, onehot = ts.synthetic_batch(3, 5, 256, 3, dev, 0)

        def window(switch, steps=10):
            model.fused_head_concat = switch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                ts.train_step(model, opt, clip, onehot, 3, torch.bfloat16)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / steps

        for switch in (False, True):
            window(switch, 5)
        res = {False: [], True: []}
        for _ in range(a.rounds):
            for switch in (False, True):
                res[switch].append(window(switch))
        print("train step, 3 x 5 frames at 256^2, bf16 autocast, windows of 10 steps")
        off, on = report("switch off", res[False], "ms"), report("switch on", res[True], "ms")
        print(f"    on / off = {on / off:.3f}")
    model.fused_head_concat = True


if __name__ == "__main__":
    main()
