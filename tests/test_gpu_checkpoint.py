"""Exact resume on the device (vivim_amd/checkpoint.py): a Vivim on a one-block-per-stage SegFormer, drop-path 0.2 and the decode
head's dropouts active, four train steps with clipping at (1, 3, 3, 64, 64), `set_epoch` after the second, on three optimizer
routes:

    lean        fp32 parameters, LeanFusedAdamW, bf16 autocast
    fused-fp16  fp32 parameters, FusedStepAdamW, fp16 autocast: the loss scale of the device record is live
    master-bf16 parameters lowered to bf16, FusedStepAdamW(master_weights=True), bf16 autocast

Per route: A and A' are uninterrupted runs from one seed, B stops after step 2, saves, builds a new model and optimizer from
another seed (and another rate), loads, and takes the two remaining steps.  The yardstick is the uninterrupted twin, never the
code under test: A and A' have to be bit-equal first -- if they are not, the test fails saying that its precondition failed,
not the resume -- and then B has to equal A in every bit: the losses, every parameter and buffer, the moments, the record and
the masters, and the rate.  Everything runs under torch.use_deterministic_algorithms(True, warn_only=True)."""
import contextlib
import os

import pytest
import torch

import conftest

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
ROUTES = {"lean": (None, {}, BF16), "fused-fp16": (None, {"fused_step": True}, F16),
          "master-bf16": (BF16, {"fused_step": True, "master_weights": True}, BF16)}      # lowered to, make_optimizer's, autocast
STEPS, SAVE_AT, EPOCHS = 4, 2, 4
SEED, OTHER_SEED = 21, 77


def _log(line):
    print(line)
    try:
        os.makedirs(os.path.dirname(conftest._PARITY_LOG), exist_ok=True)
        with open(conftest._PARITY_LOG, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\t{line}\n")
    except OSError:
        pass


@contextlib.contextmanager
def _deterministic_algorithms():
    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=prev_warn)


@pytest.fixture(autouse=True)
def _fused_step_switch_on(monkeypatch):
    monkeypatch.delenv("VIVIM_NO_FUSED_OPTIMIZER", raising=False)


def _model(seed, cuda, lowered=None):
    """The model of tests/test_gpu_decode_head.py::_build_head's config, for training: drop-path and every dropout active."""
    from transformers import SegformerConfig, SegformerForSemanticSegmentation
    from vivim_amd.dp import freeze_unused
    from vivim_amd.optimizer import lower_params
    from vivim_amd.vivim import Vivim
    torch.manual_seed(seed)
    cfg = SegformerConfig(num_channels=3, num_encoder_blocks=4, depths=[1, 1, 1, 1], sr_ratios=[8, 4, 2, 1],
                          hidden_sizes=[64, 128, 320, 512], patch_sizes=[7, 3, 3, 3], strides=[4, 2, 2, 2],
                          num_attention_heads=[1, 2, 5, 8], mlp_ratios=[4, 4, 4, 4], decoder_hidden_size=768, num_labels=150)
    model = Vivim(in_chans=3, out_chans=3, depths=[1, 1, 1, 1], backbone=SegformerForSemanticSegmentation(cfg),
                  drop_path_rate=0.2, fused_upsample=True)
    freeze_unused(model)
    model = model.to(cuda).train()
    if lowered is not None:
        lower_params(model, lowered)
    return model


def _state(route, seed, cuda, lr=1e-4, **optimizer_kw):
    from vivim_amd import checkpoint as ck
    from vivim_amd.train_step import make_optimizer
    lowered, kw, _ = ROUTES[route]
    model = _model(seed, cuda, lowered)
    opt = make_optimizer(model, lr=lr, **(optimizer_kw or kw))
    return ck.TrainState(model, opt, schedule=ck.CosineSchedule(opt, EPOCHS))


def _steps(route, state, first, last, cuda):
    """Train steps [first, last), `set_epoch(1)` after step SAVE_AT; -> their losses as floats."""
    from vivim_amd.train_step import synthetic_batch, train_step
    losses = []
    for i in range(first, last):
        clip, onehot = synthetic_batch(1, 3, 64, 3, cuda, 9 + i)
        losses.append(float(train_step(state.model, state.optimizer, clip, onehot, 3, ROUTES[route][2], clip_grad_norm=1.0)))
        state.global_step += 1
        if state.global_step == SAVE_AT:
            state.epoch = 1
            state.schedule.set_epoch(1)
    return losses


def _tensors(state):
    """Every tensor the run leaves behind, on the host: parameters and buffers, and of the optimizer the moments, the step
    counts and, for FusedStepAdamW, the whole record and the masters."""
    out = {"model." + k: v.detach().cpu().clone() for k, v in state.model.state_dict().items()}
    sd = state.optimizer.state_dict()
    for i, st in enumerate(sd["state"]):
        for k, v in st.items():
            out["opt.%d.%s" % (i, k)] = v.detach().cpu().clone()
    if "record" in sd:
        out["opt.record"] = sd["record"].cpu().clone()
    for i, w in enumerate(sd.get("master", [])):
        if w is not None:
            out["opt.master.%d" % i] = w.detach().cpu().clone()
    return out


def _differing(a, b):
    assert set(a) == set(b)
    return [k for k in a if not (a[k].dtype == b[k].dtype and torch.equal(_bits(a[k]), _bits(b[k])))]


def _bits(t):
    """Equal bits, not equal values: a NaN equals itself, -0 is not +0."""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


_RUNS = {}


def _uninterrupted(route, cuda):
    """-> (losses, tensors, lr) of run A, after run A' of the same seed was required to equal it: computed once per route."""
    if route not in _RUNS:
        runs = []
        for _ in range(2):
            state = _state(route, SEED, cuda)
            losses = _steps(route, state, 0, STEPS, cuda)
            runs.append((losses, _tensors(state), state.optimizer.lr))
        (la, ta, _), (lb, tb, _) = runs
        bad = _differing(ta, tb)
        same = la == lb and not bad
        _log("A / A' precondition\t%s\t%s\tlosses A %s\tA' %s\t%d of %d tensors differ"
             % (route, "bit-equal" if same else "DIFFERENT", ["%.9g" % x for x in la], ["%.9g" % x for x in lb], len(bad), len(ta)))
        _RUNS[route] = (runs[0], same, "losses %s vs %s, %d of %d tensors differ (%s)" % (la, lb, len(bad), len(ta), bad[:4]))
    run, same, detail = _RUNS[route]
    if not same:
        pytest.fail("PRECONDITION failed, not the resume: two uninterrupted runs of route %r from one seed differ under "
                    "deterministic algorithms, so there is no yardstick for a resumed run: %s" % (route, detail))
    return run


def _interrupted(route, cuda, path, **load_kw):
    """Run B: SAVE_AT steps, save; new objects from another seed and another rate, load, the remaining steps."""
    from vivim_amd import checkpoint as ck
    state = _state(route, SEED, cuda)
    first = _steps(route, state, 0, SAVE_AT, cuda)
    ck.save_checkpoint(path, state)
    del state
    state = _state(route, OTHER_SEED, cuda, lr=5e-4)
    report = ck.load_checkpoint(path, state, **load_kw)
    assert state.epoch == 1 and state.global_step == SAVE_AT
    rest = _steps(route, state, SAVE_AT, STEPS, cuda)
    return state, report, first, rest


@pytest.mark.parametrize("route", list(ROUTES))
def test_resume_equals_the_uninterrupted_run(route, cuda, tmp_path):
    from vivim_amd.optimizer import FusedStepAdamW
    from vivim_amd.train_step import LeanFusedAdamW
    with _deterministic_algorithms():
        losses, tensors, lr = _uninterrupted(route, cuda)
        state, report, first, rest = _interrupted(route, cuda, str(tmp_path / "run.pt"))
    opt = state.optimizer
    assert type(opt) is (LeanFusedAdamW if route == "lean" else FusedStepAdamW)
    assert report == {"exact": True, "notes": []}
    print("route %s: losses %s, resumed %s" % (route, losses, first + rest))
    assert first == losses[:SAVE_AT]
    assert rest == losses[SAVE_AT:], "the losses of steps 3 and 4 differ after the resume"
    assert opt.lr == lr == state.schedule.lr_at(1) and lr != 1e-4 and lr != 5e-4
    got = _tensors(state)
    assert any(k.endswith("running_mean") for k in got) and any(k.endswith("exp_avg_sq") for k in got)
    assert ("opt.record" in got) == (route != "lean") and any(k.startswith("opt.master.") for k in got) == (route == "master-bf16")
    bad = _differing(got, tensors)
    assert not bad, "%d of %d tensors differ after the resume: %s" % (len(bad), len(got), bad[:8])
    if route == "fused-fp16":
        assert int(opt.step_count) + int(opt.skipped_steps) == STEPS
    if route == "master-bf16":
        assert state.model._vivim_param_dtype == BF16
        lowered = [(p, w) for p, w in zip(opt.params, opt.masters) if w is not None]
        assert len(lowered) > 20 and all(p.dtype == BF16 and w.dtype == torch.float32 for p, w in lowered)
        assert all(torch.equal(_bits(p.detach()), _bits(w.to(BF16))) for p, w in lowered)          # round to nearest even


def test_without_the_generators_the_resumed_loss_differs(cuda, tmp_path):
    """The control: drop-path, the head's dropouts and its coins draw from generators that were not restored."""
    with _deterministic_algorithms():
        losses, _, lr = _uninterrupted("lean", cuda)
        state, report, first, rest = _interrupted("lean", cuda, str(tmp_path / "run.pt"), restore_rng=False)
    assert report["exact"] is False and len(report["notes"]) == 1 and "restore_rng" in report["notes"][0]
    assert first == losses[:SAVE_AT] and state.optimizer.lr == lr
    assert rest[0] != losses[SAVE_AT]


def test_a_lean_checkpoint_loads_into_the_fused_step(cuda, tmp_path):
    from vivim_amd import checkpoint as ck
    from vivim_amd.optimizer import FusedStepAdamW
    path = str(tmp_path / "lean.pt")
    with _deterministic_algorithms():
        state = _state("lean", SEED, cuda)
        _steps("lean", state, 0, SAVE_AT, cuda)
        ck.save_checkpoint(path, state)
        want = _tensors(state)
        other = _state("lean", OTHER_SEED, cuda, fused_step=True)
        assert type(other.optimizer) is FusedStepAdamW
        report = ck.load_checkpoint(path, other)
        assert report["exact"] is False and "LeanFusedAdamW" in report["notes"][0] and "FusedStepAdamW" in report["notes"][0]
        assert int(other.optimizer.step_count) == SAVE_AT == other.global_step
        got = _tensors(other)
        moments = [k for k in want if k.endswith(("exp_avg", "exp_avg_sq")) or k.startswith("model.")]
        assert not [k for k in moments if not torch.equal(got[k], want[k])]
        loss = _steps("lean", other, SAVE_AT, SAVE_AT + 1, cuda)[0]
    assert loss == loss and abs(loss) < float("inf") and int(other.optimizer.step_count) == SAVE_AT + 1
    # torch.optim.AdamW's format is another one: refused, and nothing written
    torch_state = ck.TrainState(other.model, torch.optim.AdamW(other.optimizer.params, lr=1e-4))
    torch_state.schedule = ck.CosineSchedule(torch_state.optimizer, EPOCHS)
    before = _tensors(other)
    with pytest.raises(ValueError, match="saved by LeanFusedAdamW and cannot be read by AdamW"):
        ck.load_checkpoint(path, torch_state)
    assert not _differing(_tensors(other), before)


def test_a_tracker_continues_on_the_device(cuda, tmp_path):
    from vivim_amd import checkpoint as ck
    from vivim_amd.seg_metrics import SegMetricsTracker
    from vivim_amd.train_step import eval_step, synthetic_batch
    path = str(tmp_path / "val.pt")
    batches = [synthetic_batch(1, 3, 64, 3, cuda, 50 + i) for i in range(3)]
    with _deterministic_algorithms():                                   # the third forward runs on another model object
        state = _state("lean", SEED, cuda)
        whole, part = SegMetricsTracker(3), SegMetricsTracker(3)
        state.trackers = {"val": part}
        for i, (clip, onehot) in enumerate(batches):
            eval_step(state.model, clip, onehot, 3, tracker=whole)
            if i < 2:
                eval_step(state.model, clip, onehot, 3, tracker=part)
        ck.save_checkpoint(path, state)
        other = _state("lean", OTHER_SEED, cuda)
        other.trackers = {"val": SegMetricsTracker(3)}
        assert ck.load_checkpoint(path, other)["exact"]
        resumed = other.trackers["val"]
        assert resumed.state.is_cuda and torch.equal(resumed.state, part.state) and not resumed._fresh
        eval_step(other.model, *batches[2], 3, tracker=resumed)
    assert torch.equal(resumed.state, whole.state) and float(whole.state[:, 6].sum()) >= 9
    assert resumed.get_results() == whole.get_results()
