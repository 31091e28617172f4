"""Kernel launches of one tri-directional Mamba block (forward + backward, bf16 autocast, stage-0 shape of the bench) and of
one whole train step, by kernel name -- the step is host-bound, so launches are what it pays for.
    python tools/launch_count.py [--dim 64] [--batch 3] [--frames 5] [--hw 4096] [--step] [--fused-loss] [--backbone-layernorm]
                                  [--backbone-add-norm] [--fp16] [--clip-grad-norm X] [--fused-optimizer] [--master-weights]
                                  [--head-concat]
--fused-loss (with --step) counts the step with train_step(fused_loss=True) as well, and the loss alone (forward + backward on
the step's logits shape) both ways.  --backbone-layernorm (with --step) builds the model with fast_backbone_layernorm=True,
--backbone-add-norm with fused_backbone_add_norm=True.  --fp16 and --clip-grad-norm X (with --step) count the step under fp16
autocast with the dynamic loss scale and with gradient clipping; --fused-optimizer counts that step with
make_optimizer(fused_step=True) as well (the optimizer phase on the device: csrc/optimizer.hip), and --master-weights (with both)
counts it once more, last, with the model's Linear / Conv2d parameters lowered to the autocast dtype and
make_optimizer(fused_step=True, master_weights=True): autocast's per-parameter casts are gone.  --head-concat counts one Vivim.decode call (forward + backward, train mode, bf16
autocast, the bench's head shape) with Vivim(fused_head_concat=...) off and on."""
import argparse
import collections
import os
import sys

import torch
from torch.profiler import ProfilerActivity, profile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def launches(fn, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    names = collections.Counter()
    dur = collections.Counter()
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            names[ev.name[:90]] += 1
            dur[ev.name[:90]] += ev.device_time
    return names, dur


def show(title, names, dur, top=40):
    print(f"== {title}: {sum(names.values())} launches, {sum(dur.values()) / 1e3:.2f} ms of GPU time")
    for n, c in names.most_common(top):
        print(f"   {c:5d} {dur[n] / 1e3:8.3f} ms  {n}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--hw", type=int, default=4096)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--fused-loss", action="store_true")
    ap.add_argument("--backbone-layernorm", action="store_true")
    ap.add_argument("--backbone-add-norm", action="store_true")
    ap.add_argument("--fp16", action="store_true")
    ap.add_argument("--clip-grad-norm", type=float, default=None)
    ap.add_argument("--fused-optimizer", action="store_true")
    ap.add_argument("--master-weights", action="store_true")
    ap.add_argument("--head-concat", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from vivim_amd.mamba_simple import Mamba
    torch.manual_seed(0)
    m = Mamba(d_model=a.dim, bimamba_type="v3", nframes=a.frames).to(dev)
    x = torch.randn(a.batch, a.frames * a.hw, a.dim, device=dev, requires_grad=True)

    def block():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(x, nframes=a.frames)
        y.float().square().mean().backward()
    show(f"Mamba v3 block dim {a.dim} L {a.frames * a.hw} batch {a.batch}", *launches(block))
    if a.head_concat:
        from vivim_amd import train_step as ts
        head = ts.build_model(3, dev, fused_head_concat=True).train()
        g = torch.Generator().manual_seed(15)
        states = tuple(torch.randn(a.batch * a.frames, c, 64 >> s, 64 >> s, generator=g).to(dev)
                       for s, c in enumerate((64, 128, 320, 512)))
        for switch in (False, True):
            def decode(switch=switch):
                head.fused_head_concat = switch
                head.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    out = head.decode(states, a.batch, a.frames)
                out.float().square().mean().backward()
            show(f"Vivim.decode forward + backward, ({a.batch * a.frames}; 64^2 ... 8^2) bf16, fused_head_concat={switch}",
                 *launches(decode), top=40)
        del head, states
    if a.step:
        from vivim_amd import train_step as ts
        model = ts.build_model(3, dev, fast_backbone_layernorm=a.backbone_layernorm, fused_backbone_add_norm=a.backbone_add_norm)
        opt = ts.make_optimizer(model)
        clip, onehot = ts.synthetic_batch(a.batch, a.frames, 256, 3, dev, 0)

        amp = torch.float16 if a.fp16 else torch.bfloat16
        how = ("fp16" if a.fp16 else "bf16") + ("" if a.clip_grad_norm is None else f", clip_grad_norm={a.clip_grad_norm:g}")

        def step():
            ts.train_step(model, opt, clip, onehot, 3, amp, clip_grad_norm=a.clip_grad_norm)
        show(f"train step, {how}" + (", fast_backbone_layernorm=True" if a.backbone_layernorm else "")
             + (", fused_backbone_add_norm=True" if a.backbone_add_norm else ""), *launches(step), top=60)
        if a.fused_optimizer:
            fused_opt = ts.make_optimizer(model, fused_step=True)

            def step_fused_opt():
                ts.train_step(model, fused_opt, clip, onehot, 3, amp, clip_grad_norm=a.clip_grad_norm)
            show(f"train step, {how}, make_optimizer(fused_step=True): {fused_opt.launches_per_step} optimizer launches",
                 *launches(step_fused_opt), top=60)
        if a.fused_loss:
            from vivim_amd.seg_loss import recall_focused_loss_fused

            def step_fused():
                ts.train_step(model, opt, clip, onehot, 3, torch.bfloat16, fused_loss=True)
            show("train step, fused_loss=True", *launches(step_fused), top=60)
            logits = torch.randn(a.batch * a.frames, 3, 256, 256, device=dev, dtype=torch.bfloat16, requires_grad=True)
            target = onehot.argmax(dim=2).view(a.batch * a.frames, 256, 256)
            for title, fn in (("eager", ts.recall_focused_loss), ("fused", recall_focused_loss_fused)):
                def loss_only(fn=fn):
                    logits.grad = None
                    fn(logits, target, 3).backward()
                show(f"loss alone ({title}), forward + backward, {tuple(logits.shape)} bf16", *launches(loss_only), top=12)
        if a.master_weights and a.fused_optimizer:                    # last: it changes the model
            from vivim_amd.optimizer import lower_params
            lowered = lower_params(model, amp)
            mw_opt = ts.make_optimizer(model, fused_step=True, master_weights=True)

            def step_mw():
                ts.train_step(model, mw_opt, clip, onehot, 3, amp, clip_grad_norm=a.clip_grad_norm)
            show(f"train step, {how}, {len(lowered)} parameters lowered, make_optimizer(fused_step=True, master_weights=True): "
                 f"{mw_opt.launches_per_step} optimizer launches", *launches(step_mw), top=60)


if __name__ == "__main__":
    main()
