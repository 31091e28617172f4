"""csrc/optimizer.hip through vivim_amd.optimizer.FusedStepAdamW against the definition in fp64 on the CPU, taken from the fp32
state each step started from.  Tensor lists, input families, reference and bounds: tests/fused_optimizer_cases.py (its docstring
derives the bounds; tests/test_abi_fused_optimizer.py shows a torch fp32 restatement of the kernels inside them: p 0.54, m 0.25,
v 0.63 of the bound at worst, the norm below 1 % of its bound)."""
import copy
import os

import pytest
import torch

import conftest
import fused_optimizer_cases as oc

pytestmark = pytest.mark.gpu

HYPER = dict(lr=oc.LR, betas=oc.BETAS, eps=oc.EPS, weight_decay=oc.WD)


def _log(what, shape, ratio):
    try:
        os.makedirs(os.path.dirname(conftest._PARITY_LOG), exist_ok=True)
        with open(conftest._PARITY_LOG, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\t{what}\tfloat32\tshape={tuple(shape)}"
                    f"\tmax_err_over_bound={ratio:.3e}\n")
    except OSError:
        pass


def _offset_view(t, dev):
    """t on the device as a view one element into its storage (4 bytes off any 16-byte boundary)."""
    buf = torch.empty(t.numel() + 1, device=dev)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    return view


def _build(which, family, seed, dev):
    """-> (optimizer, parameters, layouts) of list `which`, every tensor laid out as the list says."""
    from vivim_amd.optimizer import FusedStepAdamW
    shapes = oc.shapes_of(which)
    params = []
    for (shape, layout), t in zip(shapes, oc.params_cpu(which, family, seed)):
        if layout == "p1":
            data = _offset_view(t, dev)
        elif layout == "row":
            data = torch.zeros(3, *shape, device=dev)[1]
            data.copy_(t)
            assert data.data_ptr() % 16 != 0
        else:
            data = t.to(dev)
        params.append(torch.nn.Parameter(data))
    opt = FusedStepAdamW(params, **HYPER)
    for i, (shape, layout) in enumerate(shapes):
        if layout == "m1":
            opt.exp_avg[i] = _offset_view(torch.zeros(shape), dev)
        if layout == "v1":
            opt.exp_avg_sq[i] = _offset_view(torch.zeros(shape), dev)
    opt._build_tables()                                                     # the two states above moved
    for i, (_, layout) in enumerate(shapes):
        tensor = {"p1": params[i], "m1": opt.exp_avg[i], "v1": opt.exp_avg_sq[i]}.get(layout)
        assert tensor is None or tensor.data_ptr() % 16 == 4
    return opt, params, [layout for _, layout in shapes]


def _set_grads(params, layouts, grads, dev, skip=()):
    for i, (p, layout, g) in enumerate(zip(params, layouts, grads)):
        p.grad = None if i in skip else (_offset_view(g, dev) if layout == "g1" else g.to(dev))


def _state(opt, params):
    return oc.flat64(params), oc.flat64(opt.exp_avg), oc.flat64(opt.exp_avg_sq)


def _record(opt):
    rec = opt.record.cpu()
    return rec, rec.view(torch.float32)


def _check_update(tag, before, after, g64, factor, t, worst):
    want, bounds = oc.reference(*([before[0], g64] + list(before[1:])), factor, t)
    for i, (name, got, ref, bound) in enumerate(zip("pmv", after, want, bounds)):
        ratio = oc.worst(got, ref, bound)
        worst[i] = max(worst[i], ratio)
        assert ratio <= 1.0, "%s: %s misses its bound: worst |error| / bound = %.3f" % (tag, name, ratio)


@pytest.mark.parametrize("factor_case", oc.FACTORS)
@pytest.mark.parametrize("family", list(oc.P_FAMILIES))
@pytest.mark.parametrize("which", ["A", "B"])
def test_twelve_steps_against_fp64(cuda, which, family, factor_case):
    """Every element of p, m, v after each of 12 consecutive steps; the record's norm, clip, factor, count and corrections."""
    from vivim_amd import optimizer as O
    opt, params, layouts = _build(which, family, 5, cuda)
    assert opt.launches_per_step == (3 if which == "A" else 11)            # 16 tensors: one table; 1000: five
    worst = [0.0, 0.0, 0.0]
    for step in range(oc.STEPS):
        grads = oc.grads_cpu(which, step, 5)
        _set_grads(params, layouts, grads, cuda)
        before, g64 = _state(opt, params), oc.flat64(grads)
        inv_scale = 2.0 ** -16 if factor_case == "scaled" else 1.0
        norm = oc.norm64(grads, inv_scale)
        max_norm = oc.CLIP_AT * norm if factor_case == "clip" else None
        if factor_case == "one":
            opt.step()
        else:
            opt.step(max_norm=max_norm, scaled=factor_case == "scaled")
        rec, recf = _record(opt)
        t = step + 1
        assert int(rec[O.STEP]) == t and int(rec[O.FOUND_INF]) == 0 and int(rec[O.SKIPPED]) == 0
        factor = float(recf[O.FACTOR])
        if factor_case == "one":
            assert factor == 1.0 and float(recf[O.CLIP]) == 1.0
        else:
            want_clip, want_factor = oc.factor64(norm, inv_scale, max_norm)
            assert abs(float(recf[O.NORM]) - norm) <= oc.NORM_BOUND * norm
            assert abs(float(recf[O.CLIP]) - want_clip) <= 4 * oc.U * want_clip
            assert abs(factor - want_factor) <= 4 * oc.U * want_factor
            assert (want_clip < 0.38) == (factor_case == "clip")
            assert int(rec[O.GROWTH]) == (t if factor_case == "scaled" else 0) and float(recf[O.SCALE]) == 65536.0
        bc1, bc2s = oc.bias_corrections(t)
        assert abs(float(recf[O.BC1]) - float(bc1)) <= oc.U * float(bc1) and abs(float(recf[O.BC2S]) - float(bc2s)) <= oc.U * float(bc2s)
        _check_update("step %d" % step, before, _state(opt, params), g64, factor, t, worst)
    print("worst |error| / bound: p %.2f m %.2f v %.2f" % tuple(worst))
    for name, ratio in zip("pmv", worst):
        _log("fused %s list %s %s %s" % (name, which, family, factor_case), (len(params),), ratio)


@pytest.mark.parametrize("scale", [1e-6, 1.0, 3e4])
@pytest.mark.parametrize("n", [1, 255, oc.CHUNK + 1, 1000003])
def test_norm_clip_and_factor(cuda, n, scale):
    from vivim_amd import optimizer as O
    from vivim_amd.optimizer import FusedStepAdamW
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)) * scale
    p = torch.nn.Parameter(torch.zeros(n, device=cuda))
    opt = FusedStepAdamW([p], **HYPER)
    p.grad = g.to(cuda)
    norm = oc.norm64([g])
    for max_norm in (1.0, oc.CLIP_AT * norm, 4.0 * norm + 1e-5):
        opt.step(max_norm=max_norm)
        _, recf = _record(opt)
        want_clip, want_factor = oc.factor64(norm, 1.0, max_norm)
        err = abs(float(recf[O.NORM]) - norm) / norm
        print("n %d scale %g: norm relative error %.2e of %.2e" % (n, scale, err, oc.NORM_BOUND))
        assert err <= oc.NORM_BOUND
        assert abs(float(recf[O.CLIP]) - want_clip) <= 4 * oc.U * want_clip
        assert abs(float(recf[O.FACTOR]) - want_factor) <= 4 * oc.U * want_factor
    assert float(recf[O.CLIP]) == 1.0                                       # max_norm above the norm: no clipping, exactly


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_non_finite_gradient_skips_the_step(cuda, bad, where):
    """p, m, v and the count keep their bits, the scale is halved, the growth counter zeroed, skipped_steps counts; the step after
    proceeds.  `first` is the tensor of one element."""
    from vivim_amd import optimizer as O
    opt, params, layouts = _build("A", "base", 6, cuda)
    index = {"first": 0, "middle": 10, "last": len(params) - 1}[where]
    assert params[0].numel() == 1
    _set_grads(params, layouts, oc.grads_cpu("A", 0, 6), cuda)
    opt.step(max_norm=1.0, scaled=True)
    before = [t.detach().clone() for t in params + opt.exp_avg + opt.exp_avg_sq]
    rec0, recf0 = _record(opt)
    assert int(rec0[O.STEP]) == 1 and int(rec0[O.GROWTH]) == 1
    grads = oc.grads_cpu("A", 1, 6)
    grads[index].view(-1)[grads[index].numel() // 2] = bad
    _set_grads(params, layouts, grads, cuda)
    opt.step(max_norm=1.0, scaled=True)
    rec, recf = _record(opt)
    assert all(torch.equal(a, b) for a, b in zip(before, params + opt.exp_avg + opt.exp_avg_sq))
    assert int(rec[O.STEP]) == 1 and int(rec[O.FOUND_INF]) == 1 and float(recf[O.FACTOR]) == 0.0
    assert float(recf[O.SCALE]) == 0.5 * float(recf0[O.SCALE]) == 32768.0 and int(rec[O.GROWTH]) == 0
    assert int(rec[O.SKIPPED]) == int(rec0[O.SKIPPED]) + 1 == 1
    assert int(opt.skipped_steps) == 1 and int(opt.step_count) == 1 and float(opt.loss_scale) == 32768.0
    # the step after: the new scale, a normal update
    grads = oc.grads_cpu("A", 2, 6)
    _set_grads(params, layouts, grads, cuda)
    state, g64 = _state(opt, params), oc.flat64(grads)
    opt.step(max_norm=None, scaled=True)
    rec, recf = _record(opt)
    assert int(rec[O.STEP]) == 2 and int(rec[O.FOUND_INF]) == 0 and int(rec[O.GROWTH]) == 1 and int(rec[O.SKIPPED]) == 1
    assert float(recf[O.FACTOR]) == 2.0 ** -15 and float(recf[O.SCALE]) == 32768.0
    _check_update("after the skip", state, _state(opt, params), g64, 2.0 ** -15, 2, [0.0, 0.0, 0.0])


def test_the_scale_grows_after_2000_good_steps(cuda):
    from vivim_amd import optimizer as O
    opt, params, layouts = _build("A", "base", 7, cuda)
    _set_grads(params, layouts, oc.grads_cpu("A", 0, 7), cuda)
    opt.record[O.GROWTH] = O.GROWTH_INTERVAL - 1                           # 1999 good steps so far
    opt.step(scaled=True)                                                   # the 2000th
    rec, recf = _record(opt)
    assert int(rec[O.GROWTH]) == 0 and float(recf[O.SCALE]) == 131072.0 and float(recf[O.FACTOR]) == 2.0 ** -16
    opt.record[O.GROWTH] = O.GROWTH_INTERVAL - 2                           # one short of that: counted, the scale stays
    opt.step(scaled=True)
    rec, recf = _record(opt)
    assert int(rec[O.GROWTH]) == O.GROWTH_INTERVAL - 1 == 1999 and float(recf[O.SCALE]) == 131072.0
    assert float(recf[O.FACTOR]) == 2.0 ** -17
    opt.record[O.GROWTH] = 0
    opt.step(max_norm=1e9)                                                  # not scaled: the policy rests, the factor is the clip's
    rec, recf = _record(opt)
    assert int(rec[O.GROWTH]) == 0 and float(recf[O.SCALE]) == 131072.0 and float(recf[O.FACTOR]) == 1.0 and int(rec[O.STEP]) == 3


def test_missing_gradients_new_storage_and_strided_gradients(cuda):
    from vivim_amd import optimizer as O
    opt, params, layouts = _build("A", "base", 8, cuda)
    worst = [0.0, 0.0, 0.0]
    # a parameter whose grad is None is untouched; the others move, with the one shared count
    skip = (3, 9)
    grads = oc.grads_cpu("A", 0, 8)
    _set_grads(params, layouts, grads, cuda, skip=skip)
    kept = [[t[i].detach().clone() for i in skip] for t in (params, opt.exp_avg, opt.exp_avg_sq)]
    before = _state(opt, params)
    g64 = oc.flat64([torch.zeros_like(g) if i in skip else g for i, g in enumerate(grads)])
    opt.step(max_norm=oc.CLIP_AT * oc.norm64([g for i, g in enumerate(grads) if i not in skip]))
    _, recf = _record(opt)
    after = _state(opt, params)
    for tensors, old in zip((params, opt.exp_avg, opt.exp_avg_sq), kept):
        assert all(torch.equal(tensors[i], o) for i, o in zip(skip, old))
    offsets = [0]
    for p in params:
        offsets.append(offsets[-1] + p.numel())
    live = torch.ones(offsets[-1], dtype=torch.bool)
    for i in skip:
        live[offsets[i]:offsets[i + 1]] = False
    _check_update("grad None", [b[live] for b in before], [a[live] for a in after], g64[live], float(recf[O.FACTOR]), 1, worst)
    assert not torch.equal(before[0][live], after[0][live]) and int(opt.step_count) == 1
    # all of them None: nothing happens, nothing is launched
    _set_grads(params, layouts, grads, cuda, skip=range(len(params)))
    opt.step(max_norm=1.0, scaled=True)
    assert int(opt.step_count) == 1 and all(torch.equal(a, b) for a, b in zip(after, _state(opt, params)))
    # new storage for one parameter's .data: the next step updates the new storage
    old_ptrs = list(opt._ptrs)
    params[8].data = torch.full_like(params[8], 0.25)
    grads = oc.grads_cpu("A", 1, 8)
    grads[-1] = torch.randn(7, 5, generator=torch.Generator().manual_seed(3)).t()       # a (5, 7) gradient with strides (1, 5)
    _set_grads(params, layouts, grads, cuda)
    assert not params[-1].grad.is_contiguous()
    before = _state(opt, params)
    opt.step()
    assert opt._ptrs != old_ptrs and opt._ptrs[8] == params[8].data_ptr()
    after = _state(opt, params)
    assert not bool((params[8] == 0.25).any())
    _check_update("new storage", before, after, oc.flat64(grads), 1.0, 2, worst)


def _three_steps(dev, deterministic=False, side_stream=False):
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(deterministic)
    try:
        opt, params, layouts = _build("B", "base", 9, dev)
        stream = torch.cuda.Stream(device=dev) if side_stream else torch.cuda.current_stream(dev)
        for step in range(3):
            _set_grads(params, layouts, oc.grads_cpu("B", step, 9), dev)
            stream.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(stream):
                opt.step(max_norm=1.0, scaled=True)
            torch.cuda.current_stream(dev).wait_stream(stream)
        return [t.detach().clone() for t in params + opt.exp_avg + opt.exp_avg_sq] + [opt.record.clone()]
    finally:
        torch.use_deterministic_algorithms(prev)


def test_equal_state_gives_equal_bits(cuda):
    """Twice from equal state; with torch.use_deterministic_algorithms(True), under which the route stays on; on a side stream."""
    base = _three_steps(cuda)
    assert int(base[-1][2]) == 3                                            # three steps were applied
    for kw in ({}, {"deterministic": True}, {"side_stream": True}):
        again = _three_steps(cuda, **kw)
        assert all(torch.equal(a, b) for a, b in zip(base, again)), kw


def test_no_host_synchronisation(cuda):
    opt, params, layouts = _build("B", "base", 10, cuda)
    _set_grads(params, layouts, oc.grads_cpu("B", 0, 10), cuda)
    opt.step(max_norm=1.0, scaled=True)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step(max_norm=1.0, scaled=True)
        opt.step(max_norm=1.0)
        opt.step()
        scaled_loss = torch.ones((), device=cuda) * opt.loss_scale          # what train_step does with the scale: a device op
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert int(opt.step_count) == 4 and float(scaled_loss) == 65536.0


@pytest.mark.parametrize("clip_active", [False, True])
def test_state_moves_to_the_lean_optimizer_and_back(cuda, clip_active):
    """After three fused steps the state goes into LeanFusedAdamW (clones of the parameters); the same scaled gradients are applied
    to both -- the stock side as train_step does: _foreach_mul_, clip_grad_norm_, step -- and the two results are compared with the
    fp64 definition at the fp64 factor.  Each side's allowance is the bound of fused_optimizer_cases plus what a relative error
    eps of its factor does (factor_sensitivity): eps = 0 for both when the clip is inactive (max_norm far above the norm: both
    factors are 2^-16 exactly); with an active clip eps = 4u for the fused side (pinned by the tests above) and
    NORM_BOUND + 3u for the stock side: its norm is an fp32 blocked sum too, then +1e-6, the division and the multiply in fp32."""
    from vivim_amd import optimizer as O
    from vivim_amd.train_step import LeanFusedAdamW
    opt, params, layouts = _build("A", "base", 11, cuda)
    for step in range(3):
        _set_grads(params, layouts, oc.grads_cpu("A", step, 11), cuda)
        opt.step(max_norm=1.0, scaled=True)
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    lean = LeanFusedAdamW(twins, **HYPER)
    lean.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert all(float(t) == 3.0 for t in lean.state[cuda][2])
    grads = [g * 65536.0 for g in oc.grads_cpu("A", 4, 11)]                 # scaled gradients: exact multiples
    norm = oc.norm64(grads, 2.0 ** -16)
    max_norm = oc.CLIP_AT * norm if clip_active else 1e9
    _set_grads(params, layouts, grads, cuda)
    for q, g in zip(twins, grads):
        q.grad = g.to(cuda)
    before, g64 = _state(opt, params), oc.flat64(grads)
    assert all(torch.equal(a, b) for a, b in zip(before, (oc.flat64(twins), oc.flat64(lean.state[cuda][0]), oc.flat64(lean.state[cuda][1]))))
    opt.step(max_norm=max_norm, scaled=True)
    torch._foreach_mul_([q.grad for q in twins], 1.0 / 65536.0)
    torch.nn.utils.clip_grad_norm_(twins, max_norm)
    lean.step()
    _, factor = oc.factor64(norm, 2.0 ** -16, max_norm)
    want, bounds = oc.reference(before[0], g64, before[1], before[2], factor, 4)
    sens = oc.factor_sensitivity(g64, before[1], before[2], factor, 4)
    eps_fused, eps_stock = (4 * oc.U, oc.NORM_BOUND + 3 * oc.U) if clip_active else (0.0, 0.0)
    fused = _state(opt, params)
    stock = (oc.flat64(twins), oc.flat64(lean.state[cuda][0]), oc.flat64(lean.state[cuda][1]))
    for name, f, s, w, b, d in zip("pmv", fused, stock, want, bounds, sens):
        rf, rs = oc.worst(f, w, b + eps_fused * d), oc.worst(s, w, b + eps_stock * d)
        both = oc.worst(f, s, 2 * b + (eps_fused + eps_stock) * d)
        print("%s: fused %.3f, stock %.3f of its allowance; fused - stock %.3f of the sum" % (name, rf, rs, both))
        _log("fused %s vs fp64 (clip %s)" % (name, clip_active), f.shape, rf)
        _log("stock %s vs fp64 (clip %s)" % (name, clip_active), s.shape, rs)
        assert both <= 1.0 and rf <= 1.0, (name, rf, rs, both)
    # and back: the lean optimizer's checkpoint has no record -- the largest per-parameter step becomes the count
    back_params = [torch.nn.Parameter(q.detach().clone()) for q in twins]
    back = O.FusedStepAdamW(back_params, **HYPER)
    back.load_state_dict(copy.deepcopy(lean.state_dict()))
    assert int(back.step_count) == 4 and float(back.loss_scale) == 65536.0
    assert all(torch.equal(a, b) for a, b in zip(back.exp_avg + back.exp_avg_sq, lean.state[cuda][0] + lean.state[cuda][1]))
    # its own checkpoint carries the record: a copy continues bit for bit
    copy_params = [torch.nn.Parameter(p.detach().clone()) for p in params]
    twin = O.FusedStepAdamW(copy_params, **HYPER)
    twin.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert torch.equal(twin.record, opt.record)
    grads = oc.grads_cpu("A", 5, 11)
    _set_grads(params, layouts, grads, cuda)
    for q, g in zip(copy_params, grads):
        q.grad = g.to(cuda)
    opt.step(max_norm=1.0, scaled=True)
    twin.step(max_norm=1.0, scaled=True)
    assert all(torch.equal(a, b) for a, b in zip(params + opt.exp_avg + [opt.record], copy_params + twin.exp_avg + [twin.record]))


def test_train_step_fp16_with_clipping_end_to_end(cuda, monkeypatch):
    """The small model of test_train_step_fp16_scaling_clipping_and_optimizer_state through make_optimizer(fused_step=True)."""
    from vivim_amd.optimizer import FusedStepAdamW
    from vivim_amd.train_step import _SCALERS, LeanFusedAdamW, build_model, make_optimizer, synthetic_batch, train_step
    monkeypatch.delenv("VIVIM_NO_FUSED_OPTIMIZER", raising=False)
    torch.manual_seed(21)
    model = build_model(3, cuda, mamba_kwargs={"d_state": 16, "expand": 2}, drop_path_rate=0.0)
    assert type(make_optimizer(model)) is LeanFusedAdamW
    opt = make_optimizer(model, fused_step=True)
    assert type(opt) is FusedStepAdamW and opt.lr == 1e-4 and opt.weight_decay == 1e-2
    print("launches per step: %d for %d tensors" % (opt.launches_per_step, len(opt.params)))
    scalers = dict(_SCALERS)
    start = [p.detach().clone() for p in opt.params]
    clip, onehot = synthetic_batch(1, 3, 64, 3, cuda, 9)
    losses = [float(train_step(model, opt, clip, onehot, 3, torch.float16, clip_grad_norm=1.0)) for _ in range(3)]
    assert all(l == l and abs(l) < 1e4 for l in losses) and len(set(losses)) == 3, losses
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert _SCALERS == scalers and id(opt) not in _SCALERS
    assert float(opt.last_grad_norm) > 0 and float(opt.loss_scale) > 0
    assert int(opt.step_count) + int(opt.skipped_steps) == 3 and int(opt.step_count) >= 1
    assert any(not torch.equal(a, b) for a, b in zip(start, opt.params))
    loss = float(train_step(model, opt, clip, onehot, 3, torch.bfloat16, clip_grad_norm=1.0))      # bf16: not scaled
    assert loss == loss and int(opt.step_count) + int(opt.skipped_steps) == 4
    monkeypatch.setenv("VIVIM_NO_FUSED_OPTIMIZER", "1")
    assert type(make_optimizer(model, fused_step=True)) is LeanFusedAdamW
