"""The eval-mode decode head, stock against fused (Vivim(fused_decode_head=True): vivim_amd/decode_head.py, csrc/decode_head.hip),
in one warmed process.
    python tools/decode_head_bench.py [--reps 20] [--rounds 7] [--kernel-reps 100]
`Vivim.decode` on random encoder states at the bench workload's head, (15; 64^2, 32^2, 16^2, 8^2), and at (40; 128^2, 64^2,
32^2, 16^2), under bf16 autocast and in fp32, eval mode, no grad: device events around `reps` calls, the two heads alternating
round by round, the median round with the fastest and the slowest beside it.  Then the kernel alone at the same shapes (the
folded projections already made), with its achieved bytes/s over the bytes the algorithm needs (_lib.algorithmic_bytes).  The
yardstick is the stock head of the same run."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS = (64, 128, 320, 512)
SHAPES = [(15, 64), (40, 128)]            # frames, stage-0 edge; the other stages halve it


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


def report(label, v):
    print(f"    {label:28s} {statistics.median(v):10.1f} us  (min {min(v):.1f}, max {max(v):.1f})")
    return statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kernel-reps", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_head_bench.py measures on the GPU: none found")
    from vivim_amd import _lib, decode_head
    from vivim_amd import train_step as ts
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {a.reps} calls per round, {a.rounds} rounds")
    torch.manual_seed(0)
    model = ts.build_model(3, dev, fused_decode_head=True).eval()
    bn = model.decoder.batch_norm
    with torch.no_grad():                                    # statistics of a trained head, not the initial 0 / 1
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)

    def head(states, fused):
        def run():
            model.fused_decode_head = fused
            return model.decode(states, 1, states[0].shape[0])
        return run

    for frames, edge in SHAPES:
        g = torch.Generator().manual_seed(frames)
        states = tuple(torch.randn(frames, c, edge >> s, edge >> s, generator=g).to(dev) for s, c in enumerate(DIMS))
        for amp in (torch.bfloat16, torch.float32):
            name = f"({frames}; " + ", ".join(f"{edge >> s}^2" for s in range(4)) + f") {'bf16 autocast' if amp != torch.float32 else 'fp32'}"
            with torch.no_grad(), torch.autocast("cuda", dtype=amp, enabled=amp != torch.float32):
                assert decode_head.applies(model, states)
                ys = {fused: head(states, fused)() for fused in (False, True)}
                diff = float((ys[True].float() - ys[False].float()).norm() / ys[False].float().norm())
                res = alternate({"stock": head(states, False), "fused": head(states, True)}, a.reps, a.rounds)
                # the kernel alone: the folded projections as eval_decode makes them
                cache = decode_head._folded(model)
                weights = cache["weights"][amp]
                maps = [torch.nn.functional.linear(x.flatten(2).transpose(1, 2), w).view(x.shape[0], x.shape[2], x.shape[3], -1)
                        for x, w in zip(states, weights)]
                size = tuple(states[0].shape[2:])
                out = torch.empty(frames, 3, *size, dtype=amp, device=dev)
                kern = alternate({"kernel": lambda: decode_head.fused_decode_head(maps, cache["bias"], cache["w_out"], cache["b_out"],
                                                                                   size, out=out)}, a.kernel_reps, a.rounds)
                nbytes = _lib.algorithmic_bytes("vivim_decode_head_fwd",
                                                decode_head._params(maps, cache["bias"], cache["w_out"], cache["b_out"], out, size))
            print(f"{name}: fused against stock, norm-wise {diff:.3e}")
            stock, fused = report("Vivim.decode stock", res["stock"]), report("Vivim.decode fused", res["fused"])
            print(f"    fused / stock = {fused / stock:.3f}")
            k = report("vivim_decode_head_fwd alone", kern["kernel"])
            print(f"    {nbytes / 1e6:.1f} MB algorithmic: {nbytes / k / 1e3:.1f} GB/s")
    model.fused_decode_head = True


if __name__ == "__main__":
    main()
