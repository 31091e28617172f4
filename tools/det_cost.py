"""Cost of the deterministic selective-scan backward (vivim_selective_scan_bwd_det) against the default one at the bench's
grouped stage-0 scan shapes (BASELINE.json configs 1, 2 and 4): median time of 10 calls each after 3 warm-ups, and the
slot workspace one call allocates.  Usage: python tools/det_cost.py"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import selective_scan_cuda as ss  # noqa: E402
from vivim_amd import _lib  # noqa: E402

SHAPES = [("cfg1 bf16 256^2 stage0", torch.bfloat16, 3, 384, 3, 16, 20480),
          ("cfg2 fp32 512^2 stage0", torch.float32, 8, 384, 3, 16, 81920),
          ("cfg4 dstate64 stage0", torch.bfloat16, 1, 768, 3, 64, 32768)]


def main():
    dev = torch.device("cuda:0")
    for name, dt, b, d, g, n, l in SHAPES:
        torch.manual_seed(0)
        u, dout, z = (torch.randn(b, d, l, device=dev).to(dt) for _ in range(3))
        delta = (0.2 * torch.randn(b, d, l, device=dev)).to(dt)
        A = -torch.arange(1, n + 1, dtype=torch.float32, device=dev).repeat(d, 1)
        B, C = (torch.randn(b, g, n, l, device=dev).to(dt) for _ in range(2))
        D, bias = torch.randn(d, device=dev), torch.full((d,), -4.0, device=dev)
        out, x = ss.fwd(u, delta, A, B, C, D, z, bias, True)[:2]
        dz = torch.empty_like(z)

        def call():
            ss.bwd(u, delta, A, B, C, D, z, bias, dout, x, out, dz, True, False)

        row = [name]
        for det in (False, True):
            torch.use_deterministic_algorithms(det)
            ts = []
            for i in range(13):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                torch.cuda.synchronize()
                if i >= 3:
                    ts.append(e0.elapsed_time(e1) * 1000)
            row.append(sorted(ts)[len(ts) // 2])
        torch.use_deterministic_algorithms(False)
        f = _lib.SsmFwdParams()
        f.batch, f.dim, f.n_groups, f.dstate, f.seqlen = b, d, g, n, l
        f.itype = _lib.F32 if dt == torch.float32 else _lib.BF16
        f.is_variable_B = f.is_variable_C = 1
        print(f"{row[0]:26s} default {row[1]:9.1f} us  det {row[2]:9.1f} us  ({row[2] / row[1] - 1:+.1%})  "
              f"workspace of the call {ss.last_workspace_bytes['bwd_det'] / 2**20:8.2f} MiB  "
              f"(shape-level bound {_lib.lib().vivim_scan_bwd_det_workspace_bytes(ctypes.byref(f)) / 2**20:.1f} MiB)", flush=True)
        del u, dout, z, delta, B, C, out, x, dz
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
