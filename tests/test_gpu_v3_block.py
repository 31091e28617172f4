"""GPU: the whole v3 block against an independent float64 reference (tests/v3_block_cases.py, pinned on the CPU by
test_v3_block_reference.py), at shapes where the direction maps use several workgroups, the conv takes its pipelined
kernels, the scan is cut into segments and the split-K weight gradients get the row-slice operands of the real call -- all
at once -- and at shapes where the maps take their element-wise kernel inside the block.

Each case runs three ways on the same seeded parameters and input:
    (a) the grouped path;
    (b) the grouped path with vivim_amd.wgrad.MIN_TOKENS = 0: csrc/wgrad.hip on x_dbl[:, :R] and the other operands as the
        backward passes them (16-bit operands only: an fp32 run has no such kernel and must not call it);
    (c) VIVIM_SEPARATE_DIRECTIONS=1, the reference's three-call composition.
e(p) is block_errors of path p against the float64 reference: the worst per-token relative error of y and dx, the norm-wise
relative error of every parameter gradient.  Per tensor:
    e(a) <= 2 e(c) and e(b) <= 2 e(c): the grouped path is the same arithmetic in other launch shapes; only summation order may
        differ (atomics, split-K, segment carries), and where it rounds differently it rounds less (one rounding in the combine
        in place of three, fp32 out of wgrad_nt).  The factor 2 is the margin for reordering and is not tuned;
    the reference composition itself is held to absolute caps, without which the relative bound would check nothing: in fp32
        e(c) <= 1e-3 for every tensor (BASELINE.json's north-star bound); under 16-bit autocast e(c) of y and dx within the rtol
        conftest.SCAN_CLOSE gives for that dtype.
Every figure goes into the parity log before anything is asserted.

fp32 runs take the ratio under torch.use_deterministic_algorithms.  There every error is 1-3 units of roundoff, most of it from the
order in which the scan's and the conv's float atomics land: traced on grad:D at L = 2600, the error of dD against the float64
sum of the kernel's OWN inputs is 0.8e-7 to 2.0e-7 from one run to the next on either path (its inputs are 4e-8 from the reference
on both, and g * fl(1/3) in place of g / 3 changes nothing), so e(a) / e(c) was anything from 0.6 to 2.8 on unchanged code.  The
deterministic entry points run the same kernel families and store the cross-workgroup partial sums in a fixed order
(include/vivim_hip.h), which makes e(a), e(b) and e(c) functions of the inputs; in fp32 (b) then repeats (a) bit for bit, since
csrc/wgrad.hip takes 16-bit operands only.  The default atomics run follows and is held to the absolute cap on every path.  The
16-bit runs keep their atomics: their errors are 1e-3 and more, and the order of the sums does not show in them.

fp16 runs multiply the loss by LOSS_SCALE before backward and divide the fp32 gradients by it afterwards, both exact.  A deviation
from the loss as the issue writes it, which its author should confirm: unscaled, the loss's gradient 2 y / numel is 7e-6, below
fp16's smallest normal, what follows underflows on every path (e(c) of dx 0.199 against the rtol 3e-3), and the train step that
the 16-bit runs are to mirror runs fp16 under a loss scale (vivim_amd/train_step.py, 65536 at the start).

Each run also asserts that out_proj's F.linear can view its operand as the (B L, d_inner) matrix without a copy -- the block test
found the grouped path copying there, with an fp32 out_proj.weight gradient 3.8 times further from float64 at L = 2600; since
then combine_directions returns (D, B, L) memory like the composition -- and the pinned runs assert from a kernel trace that the
lanes=channels forward and the second-generation lanes=states backward ran on every path.

Measured on an MI355X, worst over the tensors of a run: e(a) / e(c) = e(b) / e(c) at most 1.59 in fp32 (grad:dt_proj_b.bias, L = 2600:
1.77e-7 against 1.11e-7), 1.39 in bf16, 1.12 in fp16; e(c) of y / dx at most 1.7e-2 / 2.2e-2 in bf16 (rtol 3e-2) and 2.4e-3 / 2.5e-3
in fp16 (rtol 3e-3); every fp32 e(c) at most 7.4e-6."""
import contextlib
import os

import pytest
import torch

import conftest
import v3_block_cases as vc
from fp64_bounds import name as dtype_name

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
BIG = (2, 32, 16, 5, 520)                    # L = 2600, d_inner = 64: whole 64-channel blocks for the pinned families
# (B, d_model, d_state, nf, hw), dtype, (forward, backward) scan family pinned with vivim_set_tuning or None for the plan's choice
RUNS = [
    (BIG, F32, None), (BIG, BF16, None),
    (BIG, F32, (5, 5)), (BIG, BF16, (5, 5)),                 # lanes=channels forward, second-generation lanes=states backward
    ((3, 16, 16, 2, 36), BF16, None), ((3, 16, 16, 2, 36), F16, None),      # a 6x6 image: element-wise maps
    ((3, 16, 16, 8, 5), F32, None), ((3, 16, 16, 8, 5), BF16, None),        # every vector straddles a frame
    ((1, 16, 64, 17, 8), F32, None),                                        # nf > 16, d_state 64
]
PATHS = ("grouped", "grouped_splitk", "separate")
PINNED_KERNELS = ("ssm_fwd_chan_kernel", "ssm_ls2_bwd_kernel")     # what forward 5 / backward 5 launch (csrc/scan_fwd_chan.hip, scan_ls2.hip)
LOSS_SCALE = 65536.0                         # fp16 only: the scale vivim_amd.train_step starts its fp16 steps with


def _id(run):
    shape, dtype, pin = run
    return "x".join(map(str, shape)) + "-" + dtype_name(dtype) + ("-auto" if pin is None else f"-fwd{pin[0]}bwd{pin[1]}")


@pytest.fixture
def tuning():
    from vivim_amd import _lib
    L = _lib.lib()
    prev = []

    def pin(fwd=0, bwd=0):
        prev.append((L.vivim_set_tuning(0, fwd), L.vivim_set_tuning(1, bwd)))

    yield pin
    if prev:
        L.vivim_set_tuning(0, prev[0][0])
        L.vivim_set_tuning(1, prev[0][1])


_cases = {}


def _case(shape):
    """The seeded module (CPU, fp32 parameters), its input and the float64 reference of both: computed once per shape, shared by
    the dtypes and tunings of that shape, never modified."""
    if shape not in _cases:
        from mamba_ssm import Mamba
        B, d_model, d_state, nf, hw = shape
        torch.manual_seed(1234 + d_model + nf + hw)
        m = Mamba(d_model=d_model, d_state=d_state, d_conv=4, expand=2, bimamba_type="v3", nframes=nf)
        with torch.no_grad():                                  # A_log and D start equal in the three directions: tell them apart
            for sfx in ("", "_b", "_s"):
                getattr(m, f"A{sfx}_log").add_(0.1 * torch.randn(m.d_inner, d_state))
                getattr(m, "D" + sfx).add_(0.1 * torch.randn(m.d_inner))
        x = torch.randn(B, nf * hw, d_model)
        state = {k: v.detach().clone() for k, v in m.named_parameters()}
        _cases[shape] = (state, x, vc.v3_reference(x, state, nf))
    return _cases[shape]


def _log(tensor, dtype, shape, errs):
    try:
        os.makedirs(os.path.dirname(conftest._PARITY_LOG), exist_ok=True)
        with open(conftest._PARITY_LOG, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\tv3_block.{tensor}\t{dtype_name(dtype)}\tshape={shape}"
                    + "".join(f"\te_{p}={errs[p]:.3e}" for p in PATHS)
                    + f"\tgrouped_over_separate={errs['grouped'] / max(errs['separate'], 1e-300):.3f}"
                    + f"\tsplitk_over_separate={errs['grouped_splitk'] / max(errs['separate'], 1e-300):.3f}\n")
    except OSError:
        pass


@pytest.mark.parametrize("run", RUNS, ids=[_id(r) for r in RUNS])
def test_v3_block_against_fp64_reference(run, cuda, monkeypatch, tuning):
    from mamba_ssm import Mamba
    from vivim_amd import mamba_simple, wgrad
    shape, dtype, pin = run
    B, d_model, d_state, nf, hw = shape
    L = nf * hw
    assert L % 8 == 0                                          # else the module takes the three-call composition by itself
    state, x_cpu, ref = _case(shape)
    m = Mamba(d_model=d_model, d_state=d_state, d_conv=4, expand=2, bimamba_type="v3", nframes=nf)
    missing, unexpected = m.load_state_dict(state, strict=True)
    assert not missing and not unexpected
    m = m.to(cuda)
    x = x_cpu.to(cuda)
    if pin is not None:
        assert m.d_inner % 64 == 0
        tuning(*pin)

    stacked, products, operands = [], [], []
    real_stack, real_wgrad, real_linear = mamba_simple.stack_directions, wgrad.wgrad_nt, torch.nn.functional.linear
    monkeypatch.setattr(mamba_simple, "stack_directions", lambda *a, **k: (stacked.append(1), real_stack(*a, **k))[1])
    monkeypatch.setattr(wgrad, "wgrad_nt", lambda a, b: (products.append((tuple(a.shape), tuple(b.shape))), real_wgrad(a, b))[1])

    def linear(inp, weight, bias=None):
        if weight is m.out_proj.weight:                        # does the (B L, d_inner) matrix the GEMM takes alias the operand?
            operands.append(inp.reshape(B * L, m.d_inner).data_ptr() == inp.data_ptr())
        return real_linear(inp, weight, bias)

    monkeypatch.setattr(torch.nn.functional, "linear", linear)
    scale = LOSS_SCALE if dtype == F16 else 1.0

    def once():
        m.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        trace = torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) if pin else contextlib.nullcontext()
        with trace as prof:
            with torch.autocast("cuda", dtype=dtype, enabled=dtype != F32):
                y = m(xi)
            (y.float().square().mean() * scale).backward()
            torch.cuda.synchronize()
        if pin:                                                # the pinned families ran, not a fallback of the plan's
            kernels = " ".join(ev.key for ev in prof.key_averages())
            assert PINNED_KERNELS[0] in kernels and PINNED_KERNELS[1] in kernels, kernels
        assert operands.pop() and not operands                 # out_proj multiplies the block's output where it lies: no copy
        assert xi.grad.dtype == F32 and all(p.grad.dtype == F32 for p in m.parameters())    # unscaled in fp32: exact
        return {"y": y.detach().cpu(), "dx": (xi.grad / scale).cpu(),
                "grads": {k: (p.grad.detach() / scale).cpu() for k, p in m.named_parameters()}}

    def three_ways():
        errs, n = {}, len(stacked)
        products.clear()
        monkeypatch.setenv("VIVIM_SEPARATE_DIRECTIONS", "0")
        errs["grouped"] = vc.block_errors(once(), ref)
        assert len(stacked) == n + 1 and not products          # the grouped path, weight gradients by the library GEMM
        with monkeypatch.context() as mp:
            mp.setattr(wgrad, "MIN_TOKENS", 0)
            errs["grouped_splitk"] = vc.block_errors(once(), ref)
        assert len(stacked) == n + 2
        R, E = m.dt_rank, m.dt_rank + 2 * d_state
        if dtype == F32:                                       # csrc/wgrad.hip takes 16-bit operands only: in fp32 (b) repeats (a)
            assert not products
        else:                                                  # both products, on the operands of the real call
            assert products == [((3, m.d_inner, B * L), (3, R, B * L)), ((3, E, B * L), (3, m.d_inner, B * L))]
        products.clear()
        monkeypatch.setenv("VIVIM_SEPARATE_DIRECTIONS", "1")
        errs["separate"] = vc.block_errors(once(), ref)
        assert len(stacked) == n + 2 and not products          # neither the maps nor the grouped op's backward ran
        return errs

    rtol16 = None if dtype == F32 else conftest.SCAN_CLOSE[dtype][0]
    bad = []
    if dtype == F32:
        # The ratio of two fp32 errors of 1-3 units of roundoff says which way the float atomics happened to fall, not which path is
        # better (module docstring).  The fp32 runs take the ratio under torch.use_deterministic_algorithms: the same kernel families
        # with the cross-workgroup sums in a fixed order (include/vivim_hip.h), so every figure is a function of the inputs.  The
        # default atomics run follows and is held to the absolute cap.
        prev = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
        torch.use_deterministic_algorithms(True)
        try:
            errs = three_ways()
        finally:
            torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])
        atomics = three_ways()
        for tensor in atomics["separate"]:
            e = {p: atomics[p][tensor] for p in PATHS}
            _log(tensor + "[atomics]", dtype, shape, e)
            print(f"{_id(run)} {tensor} [atomics]: " + " ".join(f"e_{p}={e[p]:.3e}" for p in PATHS))
            bad += [f"{tensor}: e({p}) = {e[p]:.3e} > 1e-3 with float atomics" for p in PATHS if not e[p] <= 1e-3]
    else:
        errs = three_ways()
    for tensor in errs["separate"]:
        e = {p: errs[p][tensor] for p in PATHS}
        _log(tensor, dtype, shape, e)
        print(f"{_id(run)} {tensor}: " + " ".join(f"e_{p}={e[p]:.3e}" for p in PATHS))
        for p in PATHS[:2]:
            if not e[p] <= 2 * e["separate"]:
                bad.append(f"{tensor}: e({p}) = {e[p]:.3e} > 2 * e(separate) = {2 * e['separate']:.3e}")
        if dtype == F32 and not e["separate"] <= 1e-3:
            bad.append(f"{tensor}: e(separate) = {e['separate']:.3e} > 1e-3")
        if dtype != F32 and tensor in ("y", "dx") and not e["separate"] <= rtol16:
            bad.append(f"{tensor}: e(separate) = {e['separate']:.3e} > {rtol16:.1e}")
    assert not bad, f"{_id(run)}:\n" + "\n".join(bad)
