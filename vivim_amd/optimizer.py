"""The optimizer end of the train step on the device (csrc/optimizer.hip; include/vivim_hip.h: vivim_opt_step_params): unscale,
non-finite detection, global L2 norm, clipping, AdamW, the step counter and GradScaler's loss-scale policy in a handful of
launches and with no host synchronisation.  Opt-in: `make_optimizer(model, fused_step=True)`."""
import ctypes

import torch

from . import _lib

# the record's words (include/vivim_hip.h)
SCALE, GROWTH, STEP, NORM, FOUND_INF, FACTOR, BC1, BC2S, SKIPPED, CLIP = range(10)
GROWTH_INTERVAL = 2000


def plan(numels):
    """-> (block map rows [(tensor, chunk)], cuts [(first_tensor, count, first_block, n_blocks)]) for tensors of `numels`
    elements (each > 0): one row per OPT_CHUNK elements, tensors ascending; a cut is what one call takes."""
    rows, cuts = [], []
    for first in range(0, len(numels), _lib.OPT_MAX_TENSORS):
        count = min(_lib.OPT_MAX_TENSORS, len(numels) - first)
        first_block = len(rows)
        for ti in range(first, first + count):
            rows.extend((ti, c) for c in range(-(-numels[ti] // _lib.OPT_CHUNK)))
        cuts.append((first, count, first_block, len(rows) - first_block))
    return rows, cuts


class FusedStepAdamW:
    """AdamW whose whole step -- and what `train_step` does around it for fp16 and for gradient clipping -- runs on the device:

        step(max_norm=None, scaled=False)

    unscales the gradients by the loss scale of the device record (`scaled=True`), finds non-finite values, forms the global L2
    norm of the unscaled gradients, clips to `max_norm` as `torch.nn.utils.clip_grad_norm_`, applies AdamW (decoupled weight
    decay, `torch._fused_adamw_`'s arithmetic), advances the step counter and runs GradScaler's policy (halve on overflow and
    skip the update; double after 2000 good steps).  Two or three launches read the gradients, one workgroup finalises, two or
    three launches update: `launches_per_step` of them, no atomics, bit-repeatable, and no host synchronisation.  Without
    `max_norm` and `scaled` the pass over the gradients is left out.

    `loss_scale`, `last_grad_norm`, `skipped_steps`, `step_count` and `found_inf` are 0-dim views of the device record: reading
    one on the host is the caller's choice and the only synchronisation.  The scale starts at `init_scale` (65536, what fp16
    needs) and is only looked at by `scaled=True` steps; every other step runs with a scale of 1.  `lr` may be changed between
    steps (a host scalar, passed per step).

    Differences from `torch.optim.AdamW` / `LeanFusedAdamW`: there is ONE step counter, shared by all parameters -- a parameter
    whose `.grad` is None is left out of that step, but its bias corrections later use the shared count, where torch counts per
    parameter.  A step whose gradients hold an inf or a nan is skipped whether or not it is scaled (torch would write NaNs when
    clipping such gradients), and counted in `skipped_steps`.  `state_dict()` has `LeanFusedAdamW`'s format (every "step" is the
    shared count) plus the record, so a checkpoint moves between the two classes; loading one without a record takes the
    largest per-parameter step as the count.

    Parameters must be contiguous fp32 CUDA tensors on one device; anything else raises at construction.  A gradient that is not
    dense contiguous fp32 on that device is copied into one first.  The pointer tables are rebuilt when a parameter's storage
    moved (`Mamba._fuse` replaces storage after a `.to()`): the addresses are compared on every step."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, init_scale=65536.0):
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("FusedStepAdamW: no parameter requires a gradient")
        for p in self.params:
            if not (p.is_cuda and p.dtype == torch.float32 and p.layout == torch.strided):
                raise ValueError("FusedStepAdamW takes dense fp32 CUDA parameters, got %s on %s" % (p.dtype, p.device))
            if p.device != self.params[0].device:
                raise ValueError("FusedStepAdamW takes parameters on one device, got %s and %s" % (self.params[0].device, p.device))
            if not p.is_contiguous():
                raise ValueError("FusedStepAdamW takes contiguous parameters, got strides %s for shape %s"
                                 % (tuple(p.stride()), tuple(p.shape)))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0 and lr >= 0.0 and eps >= 0.0 and weight_decay >= 0.0):
            raise ValueError("FusedStepAdamW: bad hyper-parameters")
        self.lr, self.betas, self.eps, self.weight_decay = lr, tuple(betas), eps, weight_decay
        self.device = self.params[0].device
        self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.record = torch.zeros(_lib.OPT_STATE_WORDS, dtype=torch.int32, device=self.device)
        self._record_f = self.record.view(torch.float32)
        self._record_f[SCALE] = float(init_scale)
        self.loss_scale, self.last_grad_norm = self._record_f[SCALE], self._record_f[NORM]
        self.step_count, self.skipped_steps, self.found_inf = self.record[STEP], self.record[SKIPPED], self.record[FOUND_INF]
        self._live = [i for i, p in enumerate(self.params) if p.numel() > 0]      # an empty tensor has nothing to update
        self._ptrs = None
        self._build_tables()

    # ---- the tables: what does not change per step
    def _build_tables(self):
        ps = [self.params[i] for i in self._live]
        self._ptrs = [p.data_ptr() for p in ps]
        numels = [p.numel() for p in ps]
        rows, cuts = plan(numels)
        self.total_blocks = len(rows)
        table = [self._ptrs, [self.exp_avg[i].data_ptr() for i in self._live], [self.exp_avg_sq[i].data_ptr() for i in self._live]]
        self._tables = torch.tensor(table, dtype=torch.int64).to(self.device)                     # (3, tensors) device pointers
        self._block_map = torch.tensor(rows, dtype=torch.int32).reshape(-1, 2).to(self.device)
        self._workspace = _lib.empty((2 * self.total_blocks,), torch.float32, self.device)
        self._cuts = []
        for first, count, first_block, n_blocks in cuts:
            P = self._params_struct()
            P.count, P.first_tensor, P.first_block, P.n_blocks = count, first, first_block, n_blocks
            grads = (_lib.vp * count)()
            numel = (_lib.i64 * count)(*numels[first:first + count])
            P.grads = ctypes.cast(grads, ctypes.POINTER(_lib.vp))
            P.numel = ctypes.cast(numel, ctypes.POINTER(_lib.i64))
            self._cuts.append((P, grads, numel, first, count))
        self._fin = self._params_struct()
        self.launches_per_step = 2 * len(self._cuts) + 1

    def _params_struct(self):
        P = _lib.OptStepParams()
        P.struct_bytes = ctypes.sizeof(_lib.OptStepParams)
        P.total_blocks = self.total_blocks
        n = len(self._live)
        base = self._tables.data_ptr()
        P.params, P.exp_avg, P.exp_avg_sq = base, base + 8 * n, base + 16 * n
        P.block_map, P.state = self._block_map.data_ptr(), self.record.data_ptr()
        P.workspace, P.workspace_bytes = self._workspace.data_ptr(), 8 * self.total_blocks
        return P

    # ---- torch.optim's surface, as far as train_step and checkpoints use it
    def zero_grad(self, set_to_none=True):
        for p in self.params:
            p.grad = None

    def state_dict(self):
        """`LeanFusedAdamW.state_dict()`'s format: hyper-parameters and (exp_avg, exp_avg_sq, step) per parameter, in parameter
        order -- every step is the shared count as an fp32 scalar on the device -- plus the record."""
        step = self.step_count.to(torch.float32)
        return {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay,
                "state": [{"exp_avg": m, "exp_avg_sq": v, "step": step} for m, v in zip(self.exp_avg, self.exp_avg_sq)],
                "record": self.record}

    def load_state_dict(self, sd):
        assert len(sd["state"]) == len(self.params), "optimizer state does not match the parameter list"
        self.lr, self.betas, self.eps, self.weight_decay = sd["lr"], tuple(sd["betas"]), sd["eps"], sd["weight_decay"]
        with torch.no_grad():
            for m, v, st in zip(self.exp_avg, self.exp_avg_sq, sd["state"]):
                m.copy_(st["exp_avg"])
                v.copy_(st["exp_avg_sq"])
            if sd.get("record") is not None:
                self.record.copy_(sd["record"])
            else:                      # another class's checkpoint: the largest per-parameter count; bc1 / bc2s follow on the next step
                steps = torch.stack([torch.as_tensor(st["step"], dtype=torch.float32).to(self.device) for st in sd["state"]])
                self.record[STEP] = steps.max().to(torch.int32)

    @torch.no_grad()
    def step(self, max_norm=None, scaled=False):
        if [self.params[i].data_ptr() for i in self._live] != self._ptrs:           # a parameter's storage moved
            self._build_tables()
        dev, keep, ptrs = self.device, [], []
        for i in self._live:
            g = self.params[i].grad
            if g is None:
                ptrs.append(None)
                continue
            if not (g.dtype == torch.float32 and g.layout == torch.strided and g.device == dev and g.is_contiguous()):
                g = (g if g.layout == torch.strided else g.to_dense()).to(device=dev, dtype=torch.float32).contiguous()
                keep.append(g)                                                  # alive until the launches below are enqueued
            ptrs.append(g.data_ptr())
        if all(q is None for q in ptrs):
            return
        stats = scaled or max_norm is not None
        b1, b2 = self.betas
        for P, grads, _, first, count in self._cuts:
            grads[:] = ptrs[first:first + count]
            P.scaled, P.lr, P.beta1, P.beta2, P.eps, P.weight_decay = int(bool(scaled)), self.lr, b1, b2, self.eps, self.weight_decay
            if stats:
                _lib.launch("vivim_opt_grad_stats", P, dev)
        F = self._fin
        F.total_blocks = self.total_blocks if stats else 0
        F.scaled, F.beta1, F.beta2 = int(bool(scaled)), b1, b2
        F.has_max_norm, F.max_norm = (0, 0.0) if max_norm is None else (1, float(max_norm))
        _lib.launch("vivim_opt_finalise", F, dev)
        for P, _, _, _, _ in self._cuts:
            _lib.launch("vivim_opt_adamw", P, dev)
