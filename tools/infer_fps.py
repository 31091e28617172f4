#!/usr/bin/env python3
"""Inference frames/s of the Vivim model (the reference's inference.py:294-325, 414 times a
no_grad forward per clip without a device sync; here the timed region is bracketed by torch.cuda.synchronize()).
Also prints the allocator's peak over the timed loop (VIVIM_NO_LEAN_FWD=1: the same run on the full scan forward).
    python tools/infer_fps.py [--batch 1] [--clip-length 5] [--image-size 256] [--dtype bf16] [--iters 30] [--fused-decode-head]
--fused-decode-head: Vivim(fused_decode_head=True), the eval-mode head through csrc/decode_head.hip (decode_head.py)."""
import argparse, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vivim_amd.train_step import build_model, synthetic_batch

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--clip-length", type=int, default=5)
ap.add_argument("--image-size", type=int, default=256)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--fused-decode-head", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
amp = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
torch.manual_seed(42)
model = build_model(3, dev, mamba_kwargs={"d_state": 16, "expand": 2}, fused_decode_head=a.fused_decode_head).eval()
clip, _ = synthetic_batch(a.batch, a.clip_length, a.image_size, 3, dev, 42)
with torch.no_grad(), torch.autocast("cuda", dtype=amp, enabled=amp != torch.float32):
    for _ in range(5):
        model(clip)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        out = model(clip)
    torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / a.iters
print(json.dumps({"metric": "inference frames/sec (no_grad forward, eval)", "value": round(a.batch * a.clip_length / dt, 2),
                  "ms_per_clip_batch": round(dt * 1e3, 3), "batch": a.batch, "clip_length": a.clip_length,
                  "image_size": a.image_size, "dtype": a.dtype, "finite": bool(torch.isfinite(out).all()),
                  "max_memory_allocated_MiB": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1),
                  "fused_decode_head": a.fused_decode_head,
                  "lean_fwd": os.environ.get("VIVIM_NO_LEAN_FWD", "0") != "1"}))
