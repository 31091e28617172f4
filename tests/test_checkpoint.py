"""vivim_amd/checkpoint.py on the CPU: the cosine schedule against its formula and against torch's scheduler, exact resume of a
small torch model (Linear, BatchNorm1d, Dropout in train mode) under `torch.optim.AdamW`, the file's properties, every refusal,
the stock fp16 path's loss scale, wrapped models, the inference-side loader and a tracker.

The yardstick of a resumed run is the uninterrupted run of the same seed: every compared tensor has to be EQUAL.  The control
for the generators is the same resume with `restore_rng=False`, which has to differ."""
import math
import os

import pytest
import torch
from torch import nn

from vivim_amd import checkpoint as ck
from vivim_amd import train_step as ts

LR0 = 3e-4
STEPS, SAVE_AT, STEPS_PER_EPOCH, EPOCHS = 6, 3, 2, 3


# ---- the schedule --------------------------------------------------------------------------------------------------------------
class _HasLr:
    def __init__(self, lr):
        self.lr = lr


@pytest.mark.parametrize("epochs", [1, 10, 100])
def test_schedule_is_the_formula_bit_for_bit(epochs):
    s = ck.CosineSchedule(_HasLr(LR0), epochs)
    eta_min = LR0 * 0.01
    assert s.lr0 == LR0 and s.eta_min == eta_min
    for e in range(epochs + 1):
        assert s.lr_at(e) == eta_min + (LR0 - eta_min) * (1 + math.cos(math.pi * e / epochs)) / 2, e
    assert s.lr_at(0) == LR0 and s.lr_at(epochs) == eta_min


@pytest.mark.parametrize("epochs", [1, 10, 100])
def test_schedule_against_torchs_cosine_annealing(epochs):
    """torch's default is the recursive form, one rounding or so per epoch: epochs * 2**-50 relative."""
    p = nn.Parameter(torch.zeros(3))
    twin = torch.optim.AdamW([p], lr=LR0)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(twin, T_max=epochs, eta_min=LR0 * 0.01)
    s = ck.CosineSchedule(_HasLr(LR0), epochs)
    bound, worst = epochs * 2.0 ** -50, 0.0
    for e in range(epochs + 1):
        want = twin.param_groups[0]["lr"]
        worst = max(worst, abs(s.lr_at(e) - want) / want / bound)
        twin.step()
        sched.step()
    print("epochs %d: worst |lr_at - CosineAnnealingLR| / lr = %.3f of the bound %.3e" % (epochs, worst, bound))
    assert worst <= 1.0


def test_set_epoch_writes_the_rate():
    a, b = nn.Parameter(torch.zeros(2)), nn.Parameter(torch.zeros(2))
    opt = torch.optim.AdamW([{"params": [a]}, {"params": [b]}], lr=LR0)
    s = ck.CosineSchedule(opt, 10)
    assert s.lr0 == LR0 and s.epoch == 0
    s.set_epoch(4)
    assert [g["lr"] for g in opt.param_groups] == [s.lr_at(4)] * 2 and s.epoch == 4 and s.lr_at(4) < LR0
    stand_in = _HasLr(1e-3)
    t = ck.CosineSchedule(stand_in, 5)
    t.set_epoch(5)
    assert stand_in.lr == t.lr_at(5) == 1e-3 * 0.01 and t.epoch == 5
    u = ck.CosineSchedule(stand_in, 5, lr0=2e-3, eta_min_ratio=0.1)                  # an explicit lr0 is written at once
    assert stand_in.lr == 2e-3 and u.eta_min == 2e-3 * 0.1
    fresh = ck.CosineSchedule(_HasLr(7.0), 2)
    fresh.load_state_dict(t.state_dict())
    assert fresh.state_dict() == t.state_dict() == {"lr0": 1e-3, "epochs": 5, "eta_min": 1e-3 * 0.01, "epoch": 5}


def test_param_groups_that_disagree_are_refused():
    a, b = nn.Parameter(torch.zeros(2)), nn.Parameter(torch.zeros(2))
    opt = torch.optim.AdamW([{"params": [a], "lr": 1e-3}, {"params": [b], "lr": 2e-3}])
    with pytest.raises(ValueError, match="group 0: 0.001, group 1: 0.002"):
        ck.CosineSchedule(opt, 10)
    assert ck.CosineSchedule(opt, 10, lr0=1e-3).lr_at(0) == 1e-3


# ---- a small run -----------------------------------------------------------------------------------------------------------------
def _build(seed, lr=LR0):
    torch.manual_seed(seed)
    model = nn.Sequential(nn.Linear(8, 16), nn.BatchNorm1d(16), nn.ReLU(), nn.Dropout(0.3), nn.Linear(16, 16), nn.ReLU(),
                          nn.Linear(16, 4)).train()
    opt = ts.make_optimizer(model, lr=lr)
    assert type(opt) is torch.optim.AdamW
    state = ck.TrainState(model, opt, schedule=ck.CosineSchedule(opt, EPOCHS))
    return state


def _batch(i):
    g = torch.Generator().manual_seed(1000 + i)
    return torch.randn(5, 8, generator=g), torch.randn(5, 4, generator=g)


def _steps(state, first, last, trace):
    """Steps [first, last) with `set_epoch` at every epoch's first step; appends (loss, lr) to `trace`."""
    for i in range(first, last):
        if i % STEPS_PER_EPOCH == 0:
            state.epoch = i // STEPS_PER_EPOCH
            state.schedule.set_epoch(state.epoch)
        x, y = _batch(i)
        loss = nn.functional.mse_loss(state.model(x), y)
        state.optimizer.zero_grad()
        loss.backward()
        state.optimizer.step()
        state.global_step += 1
        trace.append((loss.detach().clone(), state.optimizer.param_groups[0]["lr"]))


def _tensors(state):
    """Every tensor a run leaves behind, by name: parameters, buffers and the optimizer's moments and step counts."""
    out = {"model." + k: v.detach().clone() for k, v in state.bare_model.state_dict().items()}
    for i, st in state.optimizer.state_dict()["state"].items():
        for k, v in st.items():
            out["opt.%d.%s" % (i, k)] = torch.as_tensor(v).detach().clone()
    return out


def _assert_same(got, want):
    assert set(got) == set(want)
    bad = [k for k in want if not (got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]))]
    assert not bad, bad


@pytest.fixture(scope="module")
def uninterrupted():
    state, trace = _build(1), []
    _steps(state, 0, STEPS, trace)
    return trace, _tensors(state)


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """The same run stopped after SAVE_AT steps, in the middle of an epoch; -> (path, its trace so far)."""
    path = str(tmp_path_factory.mktemp("ckpt") / "run.pt")
    state, trace = _build(1), []
    _steps(state, 0, SAVE_AT, trace)
    state.extra = {"fold": 2, "note": "mid-epoch"}
    ck.save_checkpoint(path, state)
    return path, trace


def _resume(path, **kw):
    state = _build(99, lr=5e-3)                      # another seed, another rate: everything has to come from the file
    report = ck.load_checkpoint(path, state, **kw)
    trace = []
    _steps(state, SAVE_AT, STEPS, trace)
    return state, report, trace


def test_resume_is_exact(uninterrupted, saved):
    want_trace, want = uninterrupted
    path, first = saved
    state, report, rest = _resume(path)
    assert report == {"exact": True, "notes": []}
    assert state.global_step == STEPS and state.epoch == (STEPS - 1) // STEPS_PER_EPOCH and state.extra == {"fold": 2, "note": "mid-epoch"}
    trace = first + rest
    assert [lr for _, lr in trace] == [lr for _, lr in want_trace]
    assert len({lr for _, lr in want_trace}) == EPOCHS                   # the rate did change along the way
    assert all(torch.equal(a, b) for (a, _), (b, _) in zip(trace, want_trace)), (trace, want_trace)
    got = _tensors(state)
    assert any(k.endswith("running_var") for k in got) and any(k.endswith("exp_avg_sq") for k in got) and any(k.endswith("step") for k in got)
    _assert_same(got, want)


def test_without_the_generators_the_resume_differs(uninterrupted, saved):
    """The control: the test above sees the generator (the Dropout's mask of the first resumed step)."""
    want_trace, _ = uninterrupted
    state, report, rest = _resume(saved[0], restore_rng=False)
    assert report["exact"] is False and "restore_rng" in report["notes"][0]
    assert rest[0][1] == want_trace[SAVE_AT][1]                          # the rate is restored all the same
    assert not torch.equal(rest[0][0], want_trace[SAVE_AT][0])


# ---- the file --------------------------------------------------------------------------------------------------------------------
def test_file_loads_with_weights_only_and_has_the_documented_keys(saved):
    ckpt = torch.load(saved[0], weights_only=True)
    assert tuple(ckpt) == ck.KEYS == ("format", "version", "model", "param_dtype", "optimizer", "scaler", "schedule", "epoch",
                                      "global_step", "extra", "rng", "trackers")
    assert ckpt["format"] == "vivim-train-state" and ckpt["version"] == 1 and ckpt["param_dtype"] is None
    assert set(ckpt["optimizer"]) == {"class", "state"} and ckpt["optimizer"]["class"] == "AdamW"
    assert ckpt["scaler"] is None and ckpt["trackers"] == {} and ckpt["epoch"] == 1 and ckpt["global_step"] == SAVE_AT
    assert set(ckpt["schedule"]) == {"lr0", "epochs", "eta_min", "epoch"} and ckpt["schedule"]["epoch"] == 1
    assert set(ckpt["rng"]) == {"cpu", "cuda"} and ckpt["rng"]["cuda"] is None and ckpt["rng"]["cpu"].dtype == torch.uint8
    assert "1.running_mean" in ckpt["model"] and "1.num_batches_tracked" in ckpt["model"]
    assert not os.path.exists(saved[0] + ".tmp")


def test_a_failed_save_leaves_the_earlier_file_alone(saved, tmp_path, monkeypatch):
    path = str(tmp_path / "run.pt")
    with open(saved[0], "rb") as f:
        before = f.read()
    with open(path, "wb") as f:
        f.write(before)
    real = torch.save

    def half_written(obj, f, *a, **kw):
        real({"half": 1}, f)
        raise OSError("disk full")
    monkeypatch.setattr(torch, "save", half_written)
    with pytest.raises(OSError, match="disk full"):
        ck.save_checkpoint(path, _build(3))
    with open(path, "rb") as f:
        assert f.read() == before
    assert os.listdir(tmp_path) == ["run.pt"]


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _tampered(saved_path, tmp_path, change):
    ckpt = torch.load(saved_path, weights_only=True)
    change(ckpt)
    path = str(tmp_path / "tampered.pt")
    torch.save(ckpt, path)
    return path


def _target(with_tracker=False):
    """A state that has taken a step of its own, so that model AND optimizer have something to lose."""
    state = _build(5)
    _steps(state, 0, 1, [])
    if with_tracker:
        from vivim_amd.seg_metrics import SegMetricsTracker
        state.trackers = {"val": SegMetricsTracker(3)}
    return state


def _del_key(c):
    del c["model"]["4.bias"]


REFUSALS = {
    "unknown version": (lambda c: c.update(version=2), "version 2"),
    "unknown format": (lambda c: c.update(format="other"), "format 'other'"),
    "missing key": (_del_key, r"missing: 4\.bias"),
    "unexpected key": (lambda c: c["model"].update({"9.weight": torch.zeros(1)}), r"unexpected: 9\.weight"),
    "optimizer class": (lambda c: c["optimizer"].update({"class": "FusedStepAdamW"}), "saved by FusedStepAdamW and cannot be read by AdamW"),
    "tracker name": (lambda c: c["trackers"].update(test={"class": "SegMetricsTracker", "state": torch.zeros(3, 7), "fresh": True}),
                     r"trackers \['test'\].*\[\]"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_leave_model_and_optimizer_alone(case, saved, tmp_path):
    change, message = REFUSALS[case]
    path = _tampered(saved[0], tmp_path, change)
    state = _target()
    before, lr, rng = _tensors(state), state.optimizer.param_groups[0]["lr"], torch.get_rng_state()
    with pytest.raises(ValueError, match=message):
        ck.load_checkpoint(path, state)
    _assert_same(_tensors(state), before)
    assert state.optimizer.param_groups[0]["lr"] == lr and state.global_step == 1 and torch.equal(torch.get_rng_state(), rng)


def test_param_dtype_mismatch_is_refused(saved):
    state = _target()
    state.model._vivim_param_dtype = torch.bfloat16                      # as lower_params records it
    before = _tensors(state)
    with pytest.raises(ValueError, match="stored as float32, this model's as bfloat16.*lower_params.*raise_params"):
        ck.load_checkpoint(saved[0], state)
    with pytest.raises(ValueError, match="raise_params"):
        ck.load_model_weights(saved[0], state.model)
    _assert_same(_tensors(state), before)


def test_optimizer_of_another_length_is_refused(saved):
    state = _target()
    state.optimizer = torch.optim.AdamW(list(state.model[0].parameters()), lr=LR0)
    state.schedule = ck.CosineSchedule(state.optimizer, EPOCHS)
    before = _tensors(state)
    with pytest.raises(ValueError, match=r"saved optimizer has \[8\] parameters per group, this one \[2\]"):
        ck.load_checkpoint(saved[0], state)
    _assert_same(_tensors(state), before)


def test_tracker_of_another_class_is_refused(saved, tmp_path):
    path = _tampered(saved[0], tmp_path, lambda c: c["trackers"].update(
        val={"class": "BinaryMetricsTracker", "state": torch.zeros(10, dtype=torch.float64), "fresh": True}))
    state = _target(with_tracker=True)
    before = _tensors(state)
    with pytest.raises(ValueError, match="'val' was saved as a BinaryMetricsTracker and is a SegMetricsTracker"):
        ck.load_checkpoint(path, state)
    _assert_same(_tensors(state), before)


# ---- the stock fp16 path's loss scale ---------------------------------------------------------------------------------------------
def test_the_loss_scale_of_the_stock_fp16_path_round_trips(tmp_path, monkeypatch):
    monkeypatch.setattr(ts, "_SCALERS", {})
    path, bare = str(tmp_path / "scaled.pt"), str(tmp_path / "bare.pt")
    state = _build(1)
    ck.save_checkpoint(bare, state)
    ts._SCALERS[id(state.optimizer)] = {"scale": 1024.0, "good": 7}
    ck.save_checkpoint(path, state)
    assert torch.load(path, weights_only=True)["scaler"] == {"scale": 1024.0, "good": 7}
    other = _build(2)
    assert id(other.optimizer) != id(state.optimizer)
    ck.load_checkpoint(path, other)
    assert ts._SCALERS[id(other.optimizer)] == {"scale": 1024.0, "good": 7}
    ts._SCALERS[id(other.optimizer)]["good"] = 8                       # the entry is the new optimizer's own
    assert ts._SCALERS[id(state.optimizer)]["good"] == 7
    ck.load_checkpoint(bare, other)                                    # a file without one clears the stale entry
    assert id(other.optimizer) not in ts._SCALERS and id(state.optimizer) in ts._SCALERS


# ---- wrapped models and the inference-side loader ----------------------------------------------------------------------------------
class _Wrapped(nn.Module):
    """What dp.wrap returns, as far as a checkpoint cares: the model under `.module`."""

    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, x):
        return self.module(x)


def test_a_wrapped_model_saves_bare_keys(tmp_path):
    path = str(tmp_path / "wrapped.pt")
    inner = _build(1)
    _steps(inner, 0, 2, [])
    wrapped = ck.TrainState(_Wrapped(inner.model), inner.optimizer, schedule=inner.schedule)
    assert all(k.startswith("module.") for k in wrapped.model.state_dict())
    ck.save_checkpoint(path, wrapped)
    keys = list(torch.load(path, weights_only=True)["model"])
    assert keys == list(inner.model.state_dict()) and not any(k.startswith("module.") for k in keys)
    bare = _build(2)
    assert ck.load_checkpoint(path, bare)["exact"]
    _assert_same(_tensors(bare), _tensors(inner))
    again = _build(3)
    again.model = _Wrapped(again.model)                                 # and back into a wrapped one
    assert ck.load_checkpoint(path, again)["exact"]
    _assert_same(_tensors(again), _tensors(inner))


def test_load_model_weights_reads_three_forms(saved, tmp_path):
    want = torch.load(saved[0], weights_only=True)["model"]
    lightning = {"state_dict": {"model." + k: v for k, v in want.items()}, "epoch": 3}
    plain_path = str(tmp_path / "plain.pt")
    torch.save(dict(want), plain_path)
    for source in (lightning, dict(want), plain_path, saved[0]):
        model = _build(7).model
        result = ck.load_model_weights(source, model)
        assert not result.missing_keys and not result.unexpected_keys
        got = model.state_dict()
        assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    model = _build(7).model
    before = {k: v.clone() for k, v in model.state_dict().items()}
    extra = dict(want, **{"9.weight": torch.zeros(2)})
    with pytest.raises(ValueError, match=r"unexpected: 9\.weight"):
        ck.load_model_weights(extra, model, strict=True)
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    result = ck.load_model_weights(extra, model, strict=False)
    assert result.unexpected_keys == ["9.weight"] and all(torch.equal(v, want[k]) for k, v in model.state_dict().items())


# ---- trackers --------------------------------------------------------------------------------------------------------------------
def _val_batch(i):
    g = torch.Generator().manual_seed(300 + i)
    return torch.randn(2, 3, 9, 7, generator=g), torch.randint(0, 3, (2, 9, 7), generator=g)


def test_a_tracker_continues_where_it_was_saved(tmp_path):
    from vivim_amd.seg_metrics import SegMetricsTracker
    path = str(tmp_path / "tracked.pt")
    whole = SegMetricsTracker(3)
    for i in range(3):
        whole.update(*_val_batch(i))
    state = _build(1)
    state.trackers = {"val": SegMetricsTracker(3), "untouched": SegMetricsTracker(3)}
    for i in range(2):
        state.trackers["val"].update(*_val_batch(i))
    ck.save_checkpoint(path, state)
    entry = torch.load(path, weights_only=True)["trackers"]["val"]
    assert set(entry) == {"class", "state", "fresh"} and entry["class"] == "SegMetricsTracker" and entry["fresh"] is False
    other = _build(2)
    other.trackers = {"val": SegMetricsTracker(3), "untouched": SegMetricsTracker(3)}
    other.trackers["untouched"].update(*_val_batch(9))                  # a stale sum: the load has to zero it again
    assert ck.load_checkpoint(path, other)["exact"]
    assert other.trackers["untouched"]._fresh and not bool(other.trackers["untouched"].state.any())
    other.trackers["val"].update(*_val_batch(2))
    assert torch.equal(other.trackers["val"].state, whole.state) and float(whole.state[:, 6].sum()) > 0
    assert other.trackers["val"].get_results() == whole.get_results()
    with pytest.raises(ValueError, match="num_classes"):
        ck.load_checkpoint(path, ck.TrainState(other.model, other.optimizer, other.schedule,
                                               trackers={"val": SegMetricsTracker(4), "untouched": SegMetricsTracker(3)}))
