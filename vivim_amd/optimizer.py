"""The optimizer end of the train step on the device (csrc/optimizer.hip; include/vivim_hip.h: vivim_opt_step_params): unscale,
non-finite detection, global L2 norm, clipping, AdamW, the step counter and GradScaler's loss-scale policy in a handful of
launches and with no host synchronisation.  Opt-in: `make_optimizer(model, fused_step=True)`.

Master weights (opt-in on top: `lower_params` / `build_model(low_precision_params=...)`, then
`make_optimizer(model, fused_step=True, master_weights=True)`): the nn.Linear / nn.Conv2d parameters the model reads are stored
in the autocast dtype, their gradients arrive in that dtype, and the step keeps an fp32 master per tensor and writes the 16-bit
copy as a by-product (include/vivim_hip.h: vivim_opt_mw_params).  Autocast's per-parameter casts, forward and backward, are gone."""
import ctypes

import torch

from . import _lib

# the record's words (include/vivim_hip.h)
SCALE, GROWTH, STEP, NORM, FOUND_INF, FACTOR, BC1, BC2S, SKIPPED, CLIP = range(10)
GROWTH_INTERVAL = 2000


CLASSES = (torch.float32, torch.float16, torch.bfloat16)        # the order of the tables; a class's position is its _lib type code


def table_order(dtypes):
    """-> the permutation that lists tensors of `dtypes` by class -- fp32, then fp16, then bf16 -- and keeps the order inside one."""
    return sorted(range(len(dtypes)), key=lambda i: CLASSES.index(dtypes[i]))


def plan(numels, classes=None):
    """-> (block map rows [(tensor, chunk)], cuts [(first_tensor, count, first_block, n_blocks)]) for tensors of `numels`
    elements (each > 0): one row per OPT_CHUNK elements, tensors ascending; a cut is what one call takes.  `classes` (one value
    per tensor, equal values adjacent: `table_order`) ends a cut where the class changes: a call is homogeneous."""
    rows, cuts = [], []
    first = 0
    while first < len(numels):
        count = min(_lib.OPT_MAX_TENSORS, len(numels) - first)
        if classes is not None:
            count = next((k for k in range(1, count) if classes[first + k] != classes[first]), count)
        first_block = len(rows)
        for ti in range(first, first + count):
            rows.extend((ti, c) for c in range(-(-numels[ti] // _lib.OPT_CHUNK)))
        cuts.append((first, count, first_block, len(rows) - first_block))
        first += count
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
    moved (`Mamba._fuse` replaces storage after a `.to()`): the addresses are compared on every step.

    `master_weights=True` also takes fp16 and bf16 parameters.  Each gets an fp32 master -- `p.master_fp32` when `lower_params`
    left one there, else `p.detach().float()` -- which is what the step updates, with fp32 `exp_avg` / `exp_avg_sq`; the parameter
    itself receives the master rounded to nearest even, the value autocast would have cast an fp32 parameter to.  A gradient is
    expected in its parameter's dtype (copied into one otherwise).  The tables list the tensors by class -- fp32, fp16, bf16:
    `table_order` is that permutation of `params` -- and a launch never mixes classes, hence `launches_per_step`.  Fed the
    widened gradients in `table_order`, the fp32 route gives the same masters, moments and record, bit for bit.
    `master_params()` are the fp32 values in `params` order, and `state_dict()` gains "master"."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, init_scale=65536.0, master_weights=False):
        self.params = [p for p in params if p.requires_grad]
        self.master_weights = bool(master_weights)
        if not self.params:
            raise ValueError("FusedStepAdamW: no parameter requires a gradient")
        for p in self.params:
            if self.master_weights:
                if not (p.is_cuda and p.dtype in CLASSES and p.layout == torch.strided):
                    raise ValueError("FusedStepAdamW(master_weights=True) takes dense fp32, fp16 or bf16 CUDA parameters, got %s on %s"
                                     % (p.dtype, p.device))
            elif not (p.is_cuda and p.dtype == torch.float32 and p.layout == torch.strided):
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
        zeros = dict(dtype=torch.float32, memory_format=torch.contiguous_format)
        self.exp_avg = [torch.zeros_like(p, **zeros) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p, **zeros) for p in self.params]
        self.masters = [None if p.dtype == torch.float32 else self._master_of(p) for p in self.params]
        self.record = torch.zeros(_lib.OPT_STATE_WORDS, dtype=torch.int32, device=self.device)
        self._record_f = self.record.view(torch.float32)
        self._record_f[SCALE] = float(init_scale)
        self.loss_scale, self.last_grad_norm = self._record_f[SCALE], self._record_f[NORM]
        self.step_count, self.skipped_steps, self.found_inf = self.record[STEP], self.record[SKIPPED], self.record[FOUND_INF]
        live = [i for i, p in enumerate(self.params) if p.numel() > 0]            # an empty tensor has nothing to update
        self._live = self.table_order = [live[k] for k in table_order([self.params[i].dtype for i in live])]
        self._ptrs = None
        self._build_tables()

    @staticmethod
    def _master_of(p):
        master = getattr(p, "master_fp32", None)
        if master is None or master.shape != p.shape or master.device != p.device or master.dtype != torch.float32:
            master = p.detach().float()
        return master.contiguous()

    def _addresses(self):
        """What the tables hold: when one of them differs from `_ptrs`, a tensor moved."""
        return ([self.params[i].data_ptr() for i in self._live]
                + [self.masters[i].data_ptr() for i in self._live if self.masters[i] is not None])

    # ---- the tables: what does not change per step
    def _build_tables(self):
        ps = [self.params[i] for i in self._live]
        self._ptrs = self._addresses()
        numels = [p.numel() for p in ps]
        classes = [CLASSES.index(p.dtype) for p in ps]
        rows, cuts = plan(numels, classes)
        self.total_blocks = len(rows)
        table = [[p.data_ptr() for p in ps], [self.exp_avg[i].data_ptr() for i in self._live],
                 [self.exp_avg_sq[i].data_ptr() for i in self._live],
                 [0 if self.masters[i] is None else self.masters[i].data_ptr() for i in self._live]]
        self._tables = torch.tensor(table, dtype=torch.int64).to(self.device)                     # (4, tensors) device pointers
        self._block_map = torch.tensor(rows, dtype=torch.int32).reshape(-1, 2).to(self.device)
        self._workspace = _lib.empty((2 * self.total_blocks,), torch.float32, self.device)
        self._cuts = []
        for first, count, first_block, n_blocks in cuts:
            P = self._params_struct(classes[first])
            P.count, P.first_tensor, P.first_block, P.n_blocks = count, first, first_block, n_blocks
            grads = (_lib.vp * count)()
            numel = (_lib.i64 * count)(*numels[first:first + count])
            P.grads = ctypes.cast(grads, ctypes.POINTER(_lib.vp))
            P.numel = ctypes.cast(numel, ctypes.POINTER(_lib.i64))
            self._cuts.append((P, grads, numel, first, count))
        self._fin = self._params_struct()
        self.launches_per_step = 2 * len(self._cuts) + 1

    def _params_struct(self, cls=_lib.F32):
        """The fields that do not change per step; `cls`: the type code of a cut's tensors (fp32: the plain entry points)."""
        P = _lib.OptStepParams() if cls == _lib.F32 else _lib.OptMwParams()
        P.struct_bytes = ctypes.sizeof(P)
        P.total_blocks = self.total_blocks
        n = len(self._live)
        base = self._tables.data_ptr()
        P.params, P.exp_avg, P.exp_avg_sq = base, base + 8 * n, base + 16 * n
        P.block_map, P.state = self._block_map.data_ptr(), self.record.data_ptr()
        P.workspace, P.workspace_bytes = self._workspace.data_ptr(), 8 * self.total_blocks
        if cls != _lib.F32:
            P.masters, P.dtype = base + 24 * n, cls
        return P

    def master_params(self):
        """The fp32 values in `params` order: the master of a 16-bit parameter, an fp32 parameter itself."""
        return [p if w is None else w for p, w in zip(self.params, self.masters)]

    # ---- torch.optim's surface, as far as train_step and checkpoints use it
    def zero_grad(self, set_to_none=True):
        for p in self.params:
            p.grad = None

    def state_dict(self):
        """`LeanFusedAdamW.state_dict()`'s format: hyper-parameters and (exp_avg, exp_avg_sq, step) per parameter, in parameter
        order -- every step is the shared count as an fp32 scalar on the device -- plus the record."""
        step = self.step_count.to(torch.float32)
        sd = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay,
              "state": [{"exp_avg": m, "exp_avg_sq": v, "step": step} for m, v in zip(self.exp_avg, self.exp_avg_sq)],
              "record": self.record}
        if self.master_weights:
            sd["master"] = list(self.masters)                   # None for an fp32 parameter
        return sd

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
            saved = sd.get("master") or [None] * len(self.params)
            for p, w, src in zip(self.params, self.masters, saved):
                if w is not None:                               # a checkpoint without masters: the 16-bit parameter, widened
                    w.copy_(p.detach().float() if src is None else src)
                    p.copy_(w)                                  # round to nearest even, as the step writes it

    @torch.no_grad()
    def step(self, max_norm=None, scaled=False):
        if self._addresses() != self._ptrs:                                         # a parameter's or a master's storage moved
            self._build_tables()
        dev, keep, ptrs = self.device, [], []
        for i in self._live:
            g = self.params[i].grad
            if g is None:
                ptrs.append(None)
                continue
            want = self.params[i].dtype
            if not (g.dtype == want and g.layout == torch.strided and g.device == dev and g.is_contiguous()):
                g = (g if g.layout == torch.strided else g.to_dense()).to(device=dev, dtype=want).contiguous()
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
                _lib.launch("vivim_opt_grad_stats" + _suffix(P), P, dev)
        F = self._fin
        F.total_blocks = self.total_blocks if stats else 0
        F.scaled, F.beta1, F.beta2 = int(bool(scaled)), b1, b2
        F.has_max_norm, F.max_norm = (0, 0.0) if max_norm is None else (1, float(max_norm))
        _lib.launch("vivim_opt_finalise", F, dev)
        for P, _, _, _, _ in self._cuts:
            _lib.launch("vivim_opt_adamw" + _suffix(P), P, dev)


def _suffix(P):
    return "_mw" if isinstance(P, _lib.OptMwParams) else ""


# ---- the model's side of master weights
_KEEP_FP32 = ("MambaLayer", "_TokenDWConv2d")      # by class name: their kernels (and Mamba._fuse) take fp32 parameters


def _lowerable(model):
    """The parameters `lower_params` stores in 16 bits: weight and bias of every module whose type is exactly nn.Linear or
    nn.Conv2d, outside the subtrees of `_KEEP_FP32`.  Norms, the project's replacement modules and Mamba keep fp32."""
    out, seen = [], set()

    def walk(module):
        if type(module).__name__ in _KEEP_FP32:
            return
        if type(module) in (torch.nn.Linear, torch.nn.Conv2d):
            for p in (module.weight, module.bias):
                if p is not None and id(p) not in seen:
                    seen.add(id(p))
                    out.append(p)
        for child in module.children():
            walk(child)
    walk(model)
    return out


def lower_params(model, dtype):
    """Store the nn.Linear / nn.Conv2d parameters of `model` in `dtype` (fp16 or bf16), the autocast dtype it will run under:
    `p.master_fp32` keeps the fp32 tensor (FusedStepAdamW(master_weights=True) adopts it as the master), `p.data` becomes its
    rounded copy -- bit for bit what autocast casts an fp32 parameter to, so outputs and (widened) gradients are the stock
    ones.  Everything under a MambaLayer, every norm and the token-major depthwise convolutions stay fp32.  Records the dtype
    in `model._vivim_param_dtype`; -> the lowered parameters."""
    if dtype not in (torch.float16, torch.bfloat16):
        raise ValueError("lower_params: dtype must be torch.float16 or torch.bfloat16, got %s" % dtype)
    if getattr(model, "_vivim_param_dtype", None) is not None:
        raise ValueError("lower_params: the model's parameters are already stored in %s; raise_params first" % model._vivim_param_dtype)
    lowered = _lowerable(model)
    for p in lowered:
        if p.dtype != torch.float32:
            raise ValueError("lower_params: expected fp32 parameters, got %s" % p.dtype)
        p.master_fp32 = p.detach().clone()
        p.data = p.data.to(dtype)
    model._vivim_param_dtype = dtype
    return lowered


def raise_params(model, optimizer=None):
    """Undo `lower_params`: every lowered parameter becomes fp32 again, from `optimizer`'s masters (a
    FusedStepAdamW(master_weights=True)) where it has one, else from `p.master_fp32`.  -> the raised parameters."""
    masters = {}
    if optimizer is not None:
        masters = {id(p): w for p, w in zip(optimizer.params, optimizer.masters) if w is not None}
    raised = []
    for p in _lowerable(model):
        w = masters.get(id(p), getattr(p, "master_fp32", None))
        if w is None:
            continue
        p.data = w.detach().clone()
        p.grad = None                                           # a 16-bit gradient of the lowered parameter
        if hasattr(p, "master_fp32"):
            del p.master_fp32
        raised.append(p)
    model._vivim_param_dtype = None
    return raised


def check_autocast_dtype(model, amp_dtype):
    """A lowered model only runs under its own autocast dtype: anything else (fp32 included) would mix 16-bit parameters into
    fp32 operations, or cast them a second time."""
    stored = model.__dict__.get("_vivim_param_dtype")          # every step calls this: a dict lookup, not Module.__getattr__'s miss
    if stored is not None and stored != amp_dtype:
        raise ValueError("this model's Linear / Conv2d parameters are stored in %s (lower_params): it runs under autocast to that "
                         "dtype only, not %s; raise_params(model, optimizer) restores fp32 parameters" % (stored, amp_dtype))
