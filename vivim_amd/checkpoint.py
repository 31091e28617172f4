"""Checkpoint, exact resume and the learning-rate schedule of a training run.

The reference trains with `CosineAnnealingLR(optimizer, T_max=epochs, eta_min=initlr * 0.01)`, stepped once per epoch
(final_multiclass_training.py:517-528), resumes with `-resume_path` through Lightning's `ModelCheckpoint`, and loads weights for
inference with inference.py:load_model (:197-230).  Here that is

    CosineSchedule(optimizer, epochs)          the closed form of that schedule, for torch's optimizers and the project's
    TrainState(model, optimizer, ...)          what a run consists of
    save_checkpoint(path, state)               one file, written atomically, loadable with torch.load(weights_only=True)
    load_checkpoint(path, state)               everything back in place -- or a ValueError, never a quiet fall-back
    load_model_weights(source, model)          the inference-side loader

What makes a resume EXACT: the same optimizer class on both sides, the generators restored, and
`torch.use_deterministic_algorithms(True, warn_only=True)` around the steps (README "Determinism"): then the resumed run computes
the bits of the uninterrupted one.  What a checkpoint does NOT hold: Python's `random` and numpy's generator state (they belong
to the data loader), the data loader's position, and any mapping of SegFormer key names between transformers versions.

Nothing here is a hot path -- one file and one scalar per epoch -- so there is no kernel and no C-ABI entry point behind it."""
import math
import os

import torch

FORMAT = "vivim-train-state"
VERSION = 1
KEYS = ("format", "version", "model", "param_dtype", "optimizer", "scaler", "schedule", "epoch", "global_step", "extra", "rng",
        "trackers")
_PROJECT_OPTIMIZERS = ("LeanFusedAdamW", "FusedStepAdamW")     # the two read each other's state_dict (optimizer.FusedStepAdamW)
_DTYPE_NAMES = {None: None, torch.float16: "float16", torch.bfloat16: "bfloat16"}
_TRACKERS = ("SegMetricsTracker", "BinaryMetricsTracker")


def _is_torch_optimizer(optimizer):
    return isinstance(optimizer, torch.optim.Optimizer)


class CosineSchedule:
    """`CosineAnnealingLR(optimizer, T_max=epochs, eta_min=lr0 * eta_min_ratio)` in closed form,

        lr_at(e) = eta_min + (lr0 - eta_min) * (1 + cos(pi * e / epochs)) / 2

    in Python floats (fp64) for any integer e >= 0, for a `torch.optim.Optimizer` (every `param_groups[i]["lr"]` is written) and
    for `LeanFusedAdamW` / `FusedStepAdamW` (`optimizer.lr` is written), which torch's schedulers cannot wrap.  `lr0` defaults to
    the optimizer's current rate; torch param groups that disagree are refused.  `set_epoch(e)` is called by the training loop
    once per epoch, as the reference steps its scheduler; the constructor writes `lr_at(0)`.

    No optimizer code is involved: `LeanFusedAdamW.step` passes `self.lr` to `torch._fused_adamw_` on every call, and
    `FusedStepAdamW.step` copies `self.lr` into the argument struct of every cut (`P.lr = self.lr`) before each launch, so a rate
    written between two steps is the rate of the next one.

    torch's scheduler is recursive by default and gathers about one rounding per epoch; this form has none to gather, so the two
    agree to `epochs * 2**-50` relative (tests/test_checkpoint.py)."""

    def __init__(self, optimizer, epochs, lr0=None, eta_min_ratio=0.01):
        if int(epochs) != epochs or epochs < 1:
            raise ValueError("CosineSchedule: epochs must be a positive integer, got %r" % (epochs,))
        self.optimizer = optimizer
        self.epochs = int(epochs)
        self.lr0 = float(self._current_lr(optimizer) if lr0 is None else lr0)
        self.eta_min = self.lr0 * eta_min_ratio
        self.set_epoch(0)

    @staticmethod
    def _current_lr(optimizer):
        if not _is_torch_optimizer(optimizer):
            return optimizer.lr
        rates = [g["lr"] for g in optimizer.param_groups]
        if any(r != rates[0] for r in rates):
            raise ValueError("CosineSchedule: the optimizer's param groups disagree on lr (%s); pass lr0= to give them one rate"
                             % ", ".join("group %d: %r" % (i, r) for i, r in enumerate(rates)))
        return rates[0]

    def lr_at(self, e):
        if int(e) != e or e < 0:
            raise ValueError("CosineSchedule.lr_at: the epoch must be an integer >= 0, got %r" % (e,))
        return self.eta_min + (self.lr0 - self.eta_min) * (1 + math.cos(math.pi * e / self.epochs)) / 2

    def set_epoch(self, e):
        lr = self.lr_at(e)
        if _is_torch_optimizer(self.optimizer):
            for g in self.optimizer.param_groups:
                g["lr"] = lr
        else:
            self.optimizer.lr = lr
        self.epoch = int(e)
        return lr

    def state_dict(self):
        return {"lr0": self.lr0, "epochs": self.epochs, "eta_min": self.eta_min, "epoch": self.epoch}

    def load_state_dict(self, sd):
        self.lr0, self.epochs, self.eta_min, self.epoch = float(sd["lr0"]), int(sd["epochs"]), float(sd["eta_min"]), int(sd["epoch"])


class TrainState:
    """What a training run consists of: the model, the optimizer, optionally the schedule, the validation trackers by name
    (`SegMetricsTracker` / `BinaryMetricsTracker`) and `extra`, a dict of numbers and strings carried verbatim -- plus the two
    counters `epoch` and `global_step`, which the caller increments (`train_step` does not know them).  A model wrapped by
    `dp.wrap` is saved and loaded through its `.module`: the keys carry no `module.` prefix and a file moves between 1 and N
    ranks; which rank writes is the caller's business."""

    def __init__(self, model, optimizer, schedule=None, trackers=None, extra=None):
        self.model, self.optimizer, self.schedule = model, optimizer, schedule
        self.trackers = dict(trackers or {})
        self.extra = dict(extra or {})
        self.epoch = 0
        self.global_step = 0

    @property
    def bare_model(self):
        inner = getattr(self.model, "module", None)
        return inner if isinstance(inner, torch.nn.Module) else self.model


def _param_dtype_name(model):
    dtype = getattr(model, "_vivim_param_dtype", None)
    if dtype not in _DTYPE_NAMES:
        raise ValueError("checkpoint: the model's _vivim_param_dtype is %r; expected None, torch.float16 or torch.bfloat16" % (dtype,))
    return _DTYPE_NAMES[dtype]


def _model_device(model):
    p = next(iter(model.parameters()), None)
    return torch.device("cpu") if p is None else p.device


def _scalers():
    from . import train_step
    return train_step._SCALERS


def _tracker_entry(tracker):
    # reset() makes `state` and `_fresh`: nothing else is the tracker's
    return {"class": type(tracker).__name__, "state": tracker.state.clone(), "fresh": bool(tracker._fresh)}


def save_checkpoint(path, state):
    """Write `state` (a TrainState) to `path`: one `torch.save` of one dict to `path + ".tmp"`, moved into place with
    `os.replace`.  If anything raises, `path` is what it was and the temporary file is gone.  The dict holds tensors, numbers,
    strings, lists, tuples, dicts and None only (`torch.load(path, weights_only=True)` reads it):

        format, version     "vivim-train-state", 1
        model               model.state_dict() -- BatchNorm's running statistics included; a lowered model's 16-bit parameters as stored
        param_dtype         None, "float16" or "bfloat16" (model._vivim_param_dtype)
        optimizer           {"class", "state": optimizer.state_dict()} -- FusedStepAdamW's holds the device record and the masters
        scaler              train_step's loss scale of the stock fp16 path for this optimizer, {"scale", "good"}, or None
        schedule            schedule.state_dict() or None
        epoch, global_step, extra
        rng                 {"cpu": torch.get_rng_state(), "cuda": torch.cuda.get_rng_state(the model's device) or None}
        trackers            per name {"class", "state", "fresh"}

    Python's `random` and numpy's generator belong to the data loader and are not saved."""
    model = state.bare_model
    device = _model_device(model)
    scaler = _scalers().get(id(state.optimizer))
    schedule = state.schedule
    ckpt = {
        "format": FORMAT, "version": VERSION,
        "model": model.state_dict(),
        "param_dtype": _param_dtype_name(model),
        "optimizer": {"class": type(state.optimizer).__name__, "state": state.optimizer.state_dict()},
        "scaler": None if scaler is None else {"scale": float(scaler["scale"]), "good": int(scaler["good"])},
        "schedule": None if schedule is None else schedule.state_dict(),
        "epoch": int(state.epoch), "global_step": int(state.global_step), "extra": dict(state.extra),
        "rng": {"cpu": torch.get_rng_state(), "cuda": torch.cuda.get_rng_state(device) if device.type == "cuda" else None},
        "trackers": {name: _tracker_entry(t) for name, t in state.trackers.items()},
    }
    path = os.fspath(path)
    tmp = path + ".tmp"
    try:
        torch.save(ckpt, tmp)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def _first(names, n=5):
    names = sorted(names)
    return ", ".join(names[:n]) + (" ... (%d in all)" % len(names) if len(names) > n else "")


def _check_model(saved, model, what):
    """Missing, unexpected and mis-shaped keys, before anything is written (load_state_dict would stop half way)."""
    own = model.state_dict()
    missing, unexpected = set(own) - set(saved), set(saved) - set(own)
    if missing or unexpected:
        parts = []
        if missing:
            parts.append("missing: " + _first(missing))
        if unexpected:
            parts.append("unexpected: " + _first(unexpected))
        raise ValueError("%s: the saved model does not fit this one (%s); build the model with the configuration it was saved from"
                         % (what, "; ".join(parts)))
    shapes = [k for k in own if tuple(own[k].shape) != tuple(saved[k].shape)]
    if shapes:
        raise ValueError("%s: saved tensors of another shape (%s); build the model with the configuration it was saved from"
                         % (what, _first("%s %s vs %s" % (k, tuple(saved[k].shape), tuple(own[k].shape)) for k in shapes)))


def _check_param_dtype(saved, model, what):
    have = _param_dtype_name(model)
    if saved != have:
        raise ValueError("%s: the file's parameters are stored as %s, this model's as %s; bring the model to the file's form first "
                         "(lower_params(model, dtype) for a 16-bit file, raise_params(model) for an fp32 one)"
                         % (what, saved or "float32", have or "float32"))


def _check_optimizer(entry, optimizer):
    """-> a note when the load is allowed but not exact, else None."""
    saved, have = entry["class"], type(optimizer).__name__
    note = None
    if saved != have:
        if not (saved in _PROJECT_OPTIMIZERS and have in _PROJECT_OPTIMIZERS):
            raise ValueError("load_checkpoint: the optimizer state was saved by %s and cannot be read by %s (only %s read each "
                             "other's format); construct the optimizer the run was saved with" % (saved, have, " and ".join(_PROJECT_OPTIMIZERS)))
        note = "optimizer state of %s loaded into %s: the step counters and the loss-scale record do not carry over bit for bit" % (saved, have)
    sd = entry["state"]
    if _is_torch_optimizer(optimizer):
        want = [[tuple(p.shape) for p in g["params"]] for g in optimizer.param_groups]
        got = [len(g["params"]) for g in sd["param_groups"]]
        if got != [len(g) for g in want]:
            raise ValueError("load_checkpoint: the saved optimizer has %s parameters per group, this one %s; give the optimizer the "
                             "parameter list it was saved with" % (got, [len(g) for g in want]))
        shapes = [s for g in want for s in g]
        saved_ids = [i for g in sd["param_groups"] for i in g["params"]]
        moments = [sd["state"].get(i, {}).get("exp_avg") for i in saved_ids]          # None before a parameter's first step
        bad = [i for i, m, s in zip(saved_ids, moments, shapes) if m is not None and tuple(m.shape) != s]
    else:
        if len(sd["state"]) != len(optimizer.params):
            raise ValueError("load_checkpoint: the saved optimizer state has %d entries, this optimizer %d parameters; give the "
                             "optimizer the parameter list it was saved with (same model, same frozen parameters)"
                             % (len(sd["state"]), len(optimizer.params)))
        bad = [i for i, (p, st) in enumerate(zip(optimizer.params, sd["state"])) if tuple(st["exp_avg"].shape) != tuple(p.shape)]
        masters = sd.get("master")
        if masters is not None and getattr(optimizer, "masters", None) is not None:
            bad += [i for i, (p, w) in enumerate(zip(optimizer.params, masters)) if w is not None and tuple(w.shape) != tuple(p.shape)]
    if bad:
        raise ValueError("load_checkpoint: the saved optimizer state of parameter(s) %s has another shape; give the optimizer the "
                         "parameter list it was saved with" % bad[:5])
    return note


def _check_trackers(saved, trackers):
    if set(saved) != set(trackers):
        raise ValueError("load_checkpoint: the file holds the trackers %s, the state %s; pass the trackers the run was saved with, "
                         "under the same names" % (sorted(saved), sorted(trackers)))
    for name, t in trackers.items():
        if saved[name]["class"] != type(t).__name__:
            raise ValueError("load_checkpoint: tracker %r was saved as a %s and is a %s here" % (name, saved[name]["class"], type(t).__name__))
        if tuple(saved[name]["state"].shape) != tuple(t.state.shape):
            raise ValueError("load_checkpoint: tracker %r was saved with a state of shape %s, this one has %s (another num_classes?)"
                             % (name, tuple(saved[name]["state"].shape), tuple(t.state.shape)))


def _read(path, map_location):
    return torch.load(os.fspath(path), map_location=map_location, weights_only=True)


def load_checkpoint(path, state, *, restore_rng=True, map_location=None):
    """Restore `state` (a TrainState over freshly constructed objects) from `path`, in place; -> {"exact": bool, "notes": [...]}.
    `exact` says that a run continued from here computes what the saved run would have (given deterministic algorithms).

    All checks come first, and each failure is a ValueError that names the mismatch and the remedy and leaves model and
    optimizer as they were: an unknown `format` / `version`; a `param_dtype` other than the model's; missing, unexpected or
    mis-shaped model keys; an optimizer state of another length; a tracker name or class that does not match; and an optimizer
    class that cannot read the saved one -- `torch.optim.AdamW` against `LeanFusedAdamW` / `FusedStepAdamW`.  Those two read each
    other's format, so that load is made and reported as not exact.

    Then, in this order: `model.load_state_dict(strict=True)` (a copy in place: Mamba's fused views and the decode head's fold
    cache see it as any other load); `optimizer.load_state_dict` (FusedStepAdamW restores the masters and rewrites each 16-bit
    parameter from its master, so it has to follow the model); the stock fp16 path's loss scale in `train_step._SCALERS` under
    THIS optimizer's id -- a file without one removes a stale entry; the schedule, followed by `set_epoch` of its own epoch so
    that the optimizer's rate is the schedule's, not its constructor's; the counters and `extra`; the trackers; and last the
    generators (`restore_rng=False` leaves them alone and is reported as not exact).  `map_location` is torch.load's."""
    ckpt = _read(path, map_location)
    if not isinstance(ckpt, dict) or ckpt.get("format") != FORMAT:
        raise ValueError("load_checkpoint: %s is not a %r file (format %r); load_model_weights reads plain and Lightning state dicts"
                         % (path, FORMAT, ckpt.get("format") if isinstance(ckpt, dict) else type(ckpt).__name__))
    if ckpt.get("version") != VERSION:
        raise ValueError("load_checkpoint: %s has version %r, this code reads version %d; load it with the code that wrote it"
                         % (path, ckpt.get("version"), VERSION))
    model, optimizer, schedule = state.bare_model, state.optimizer, state.schedule
    notes = []
    _check_param_dtype(ckpt["param_dtype"], model, "load_checkpoint")
    _check_model(ckpt["model"], model, "load_checkpoint")
    note = _check_optimizer(ckpt["optimizer"], optimizer)
    if note:
        notes.append(note)
    _check_trackers(ckpt["trackers"], state.trackers)
    if (ckpt["schedule"] is None) != (schedule is None):
        raise ValueError("load_checkpoint: the file %s a schedule and the state %s; construct the state as the run was saved"
                         % ("holds" if ckpt["schedule"] is not None else "holds no", "has one" if schedule is not None else "has none"))

    model.load_state_dict(ckpt["model"], strict=True)
    optimizer.load_state_dict(ckpt["optimizer"]["state"])
    scalers = _scalers()
    if ckpt["scaler"] is not None:
        scalers[id(optimizer)] = {"scale": float(ckpt["scaler"]["scale"]), "good": int(ckpt["scaler"]["good"])}
    else:
        scalers.pop(id(optimizer), None)
    if schedule is not None:
        schedule.load_state_dict(ckpt["schedule"])
        schedule.set_epoch(schedule.epoch)
    state.epoch, state.global_step = int(ckpt["epoch"]), int(ckpt["global_step"])
    state.extra = dict(ckpt["extra"])
    for name, t in state.trackers.items():
        entry = ckpt["trackers"][name]
        t.state = entry["state"].clone()
        t._fresh = bool(entry["fresh"])
    device = _model_device(model)
    if not restore_rng:
        notes.append("restore_rng=False: the generators were left alone, dropout and drop-path draw other numbers")
    else:
        torch.set_rng_state(ckpt["rng"]["cpu"].cpu())
        if device.type == "cuda":
            if ckpt["rng"]["cuda"] is None:
                notes.append("the file was saved from a CPU model and holds no CUDA generator state")
            else:
                torch.cuda.set_rng_state(ckpt["rng"]["cuda"].cpu(), device)
        elif ckpt["rng"]["cuda"] is not None:
            notes.append("the file holds a CUDA generator state and the model is on the CPU: not restored")
    return {"exact": not notes, "notes": notes}


def load_model_weights(source, model, strict=True):
    """The inference-side loader (the reference's inference.py:197-230): `source` is a path or a dict.  A dict with a
    "state_dict" entry is a Lightning checkpoint, whose keys lose their `model.` prefix; a "vivim-train-state" file contributes
    its `model` entry (and its `param_dtype` is checked against the model's); anything else is a plain state dict.  A model whose
    parameters `lower_params` stored in 16 bits is refused for the other two forms: they hold fp32 weights, `raise_params` first.
    `strict` is `load_state_dict`'s, and a mismatch is a ValueError before anything is written.  SegFormer's key names differ
    between transformers 4.x and 5.x; no mapping is made here.  -> load_state_dict's result."""
    what = "load_model_weights"
    ckpt = source if isinstance(source, dict) else _read(source, "cpu")
    if not isinstance(ckpt, dict):
        raise ValueError("%s: expected a dict of tensors, a Lightning checkpoint or a %r file, got %s" % (what, FORMAT, type(ckpt).__name__))
    inner = getattr(model, "module", None)
    model = inner if isinstance(inner, torch.nn.Module) else model
    if ckpt.get("format") == FORMAT:
        if ckpt.get("version") != VERSION:
            raise ValueError("%s: the file has version %r, this code reads version %d" % (what, ckpt.get("version"), VERSION))
        _check_param_dtype(ckpt["param_dtype"], model, what)
        sd = ckpt["model"]
    else:
        if "state_dict" in ckpt and isinstance(ckpt["state_dict"], dict):
            sd = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in ckpt["state_dict"].items()}
        else:
            sd = ckpt
        _check_param_dtype(None, model, what)
    if strict:
        _check_model(sd, model, what)
    else:
        own = model.state_dict()
        bad = [k for k in sd if k in own and tuple(sd[k].shape) != tuple(own[k].shape)]
        if bad:
            raise ValueError("%s: saved tensors of another shape (%s)" % (what, _first(bad)))
    return model.load_state_dict(sd, strict=strict)
