"""CPU: the fused clip + AdamW step's entry points (include/vivim_hip.h: vivim_opt_step_params) are declared, exported and
present without disturbing the binding's tables; every bad argument is refused on the host before any launch, with its text;
FusedStepAdamW refuses what it does not take; make_optimizer's default is what it was; and a torch fp32 restatement of the kernels'
arithmetic meets the bounds of tests/test_gpu_fused_optimizer.py on that test's own inputs (fused_optimizer_cases.py)."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

import fused_optimizer_cases as oc
from conftest import ROOT
from vivim_amd import _lib, optimizer

STATS, FIN, ADAMW, QUERY = "vivim_opt_grad_stats", "vivim_opt_finalise", "vivim_opt_adamw", "vivim_opt_step_workspace_bytes"
LAUNCHING = (STATS, FIN, ADAMW)
OK, INVALID = 0, 1
PTR = 1 << 20                                    # a non-null, 16-byte aligned address: no check may dereference it


def _params(count=3, numels=(5, 4097, 1), total_blocks=4):
    """A call every entry point accepts up to the launch: the host arrays are real, the device pointers are not memory."""
    P = _lib.OptStepParams()
    P.struct_bytes = ctypes.sizeof(_lib.OptStepParams)
    P.count, P.first_tensor, P.first_block, P.n_blocks, P.total_blocks = count, 0, 0, total_blocks, total_blocks
    P.scaled, P.has_max_norm, P.max_norm = 1, 1, 1.0
    P.lr, P.beta1, P.beta2, P.eps, P.weight_decay = 1e-3, 0.9, 0.999, 1e-8, 1e-2
    n = max(count, 1)
    grads = (_lib.vp * n)(*([PTR] * n))
    numel = (_lib.i64 * n)(*(list(numels) + [1] * n)[:n])
    P.grads, P.numel = ctypes.cast(grads, ctypes.POINTER(_lib.vp)), ctypes.cast(numel, ctypes.POINTER(_lib.i64))
    P._keep = (grads, numel)
    for f in ("params", "exp_avg", "exp_avg_sq", "block_map", "state", "workspace"):
        setattr(P, f, PTR)
    P.workspace_bytes = 8 * total_blocks
    return P


def _refused(name, P, message, code=INVALID):
    """`code` and `message` through the ctypes function and, as a RuntimeError with the same text, through _lib.call; nothing is
    launched (the pointers are not memory: a kernel that started would not return an error code)."""
    L = _lib.lib()
    assert getattr(L, name)(ctypes.byref(P), None) == code, L.vivim_last_error()
    direct = L.vivim_last_error().decode()
    assert message in direct, direct
    with pytest.raises(RuntimeError) as info:
        _lib.call(name, P, 0)
    assert str(info.value) == direct
    return direct


def test_symbols_declared_exported_and_present():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vivim_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vivim_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    for name in LAUNCHING + (QUERY,):
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert "vivim_opt_step_params" in text
    for name in LAUNCHING:
        assert getattr(L, name).argtypes == [ctypes.POINTER(_lib.OptStepParams), ctypes.c_void_p]
    assert getattr(L, QUERY).argtypes == [ctypes.POINTER(_lib.OptStepParams)] and getattr(L, QUERY).restype is ctypes.c_size_t
    for define, value in (("VIVIM_OPT_CHUNK", _lib.OPT_CHUNK), ("VIVIM_OPT_MAX_TENSORS", _lib.OPT_MAX_TENSORS),
                          ("VIVIM_OPT_STATE_WORDS", _lib.OPT_STATE_WORDS)):
        assert int(re.search(r"#define %s (\d+)" % define, text).group(1)) == value
    assert (oc.CHUNK, oc.MAX_TENSORS) == (_lib.OPT_CHUNK, _lib.OPT_MAX_TENSORS)
    assert 16 * _lib.OPT_MAX_TENSORS + 128 <= 4096                        # the by-value table and its header: 4 KB of arguments


def test_the_tables_are_undisturbed():
    L = _lib.lib()
    assert L.vivim_abi_version() == 8
    assert len(_lib.STRUCTS) == 15 and _lib.OptStepParams not in _lib.STRUCTS
    assert L.vivim_sizeof(15) == 0
    for name in LAUNCHING:
        e = _lib.ENTRY_POINTS[name]
        assert e.struct is None and e.extra == (ctypes.POINTER(_lib.OptStepParams),) and e.stream and e.restype is ctypes.c_int
    e = _lib.ENTRY_POINTS[QUERY]
    assert e.struct is None and e.extra == (ctypes.POINTER(_lib.OptStepParams),) and not e.stream and e.restype is ctypes.c_size_t
    assert len([n for n, e in _lib.ENTRY_POINTS.items() if e.struct is not None and e.stream]) == 24
    assert [f[0] for f in _lib.OptStepParams._fields_] == [
        "struct_bytes", "count", "first_tensor", "first_block", "n_blocks", "total_blocks", "scaled", "has_max_norm", "max_norm",
        "lr", "beta1", "beta2", "eps", "weight_decay", "grads", "numel", "params", "exp_avg", "exp_avg_sq", "block_map", "state",
        "workspace", "workspace_bytes"]
    assert ctypes.sizeof(_lib.OptStepParams) == 8 * 4 + 6 * 8 + 8 * 8 + 8


def test_null_struct_and_struct_bytes():
    L = _lib.lib()
    size = ctypes.sizeof(_lib.OptStepParams)
    for name in LAUNCHING:
        assert getattr(L, name)(None, None) == INVALID and b"check failed" in L.vivim_last_error()
        for bad in (size - 1, size + 8, 0):
            P = _params()
            P.struct_bytes = bad
            _refused(name, P, "struct_bytes = %d" % bad)
    P = _params()
    P.struct_bytes = size - 8
    assert L.vivim_opt_step_workspace_bytes(ctypes.byref(P)) == 0 and L.vivim_opt_step_workspace_bytes(None) == 0


def test_null_tables():
    for name in LAUNCHING:
        P = _params()
        P.state = None
        _refused(name, P, "check failed")
    for field in ("params", "exp_avg", "exp_avg_sq"):
        P = _params()
        setattr(P, field, None)
        _refused(ADAMW, P, "check failed")
    for name in (STATS, ADAMW):
        P = _params()
        P.block_map = None
        _refused(name, P, "check failed")
        for field, typ in (("grads", _lib.vp), ("numel", _lib.i64)):
            P = _params()
            setattr(P, field, ctypes.POINTER(typ)())
            _refused(name, P, "check failed")


def test_counts_element_counts_and_map_rows():
    for name in (STATS, ADAMW):
        for bad in (0, -1, _lib.OPT_MAX_TENSORS + 1):
            P = _params()
            P.count = bad
            _refused(name, P, "count = %d" % bad)
        _refused(name, _params(numels=(5, 0, 1)), "numel[1] = 0")
        _refused(name, _params(numels=(5, 7, -3)), "numel[2] = -3")
        for first, n, total in ((0, 0, 4), (-1, 2, 4), (3, 2, 4), (0, 5, 4)):
            P = _params()
            P.first_block, P.n_blocks, P.total_blocks = first, n, total
            _refused(name, P, "map rows %d .. %d + %d of %d" % (first, first, n, total))
        P = _params()
        P.first_tensor = -1
        _refused(name, P, "check failed")
    for name in LAUNCHING:
        P = _params()
        P.total_blocks = -1
        _refused(name, P, "total_blocks = -1")
    P = _params(count=_lib.OPT_MAX_TENSORS, numels=())                     # the cap itself passes the count check
    P.workspace = None
    _refused(STATS, P, "workspace of")


def test_workspace_and_hyper_parameters():
    for name in (STATS, FIN):
        P = _params()
        P.workspace = None
        _refused(name, P, "workspace of 32 bytes at (nil)")
        P = _params()
        P.workspace_bytes = 31
        _refused(name, P, "workspace of 31 bytes at 0x100000: need a 8-byte aligned one of vivim_opt_step_workspace_bytes() = 32")
        P = _params()
        P.workspace = PTR + 4
        _refused(name, P, "workspace of 32 bytes")
    for name in (FIN, ADAMW):
        for b1, b2 in ((1.0, 0.999), (0.9, -0.1), (float("nan"), 0.5)):
            P = _params()
            P.beta1, P.beta2 = b1, b2
            _refused(name, P, "betas = ")
    P = _params()
    P.max_norm = -1.0
    _refused(FIN, P, "max_norm = -1")
    P = _params()
    P.lr = -1e-3
    _refused(ADAMW, P, "lr = -0.001")


def test_workspace_formula_and_bytes():
    L = _lib.lib()
    for total in (1, 4, 11500):
        assert L.vivim_opt_step_workspace_bytes(ctypes.byref(_params(total_blocks=total))) == 8 * total
    assert L.vivim_opt_step_workspace_bytes(ctypes.byref(_params(total_blocks=0))) == 0
    P = _params()                                                          # 5 + 4097 + 1 elements, 4 map rows
    assert _lib.algorithmic_bytes(STATS, P) == 4 * 4103 + 8 * 4
    assert _lib.algorithmic_bytes(ADAMW, P) == 28 * 4103                   # p, m, v read and written, g read
    assert _lib.algorithmic_bytes(FIN, P) == 8 * 4 + 4 * _lib.OPT_STATE_WORDS
    P._keep[0][1] = None                                                   # a tensor without a gradient moves nothing
    assert _lib.algorithmic_bytes(STATS, P) == 4 * 6 + 8 * 4 and _lib.algorithmic_bytes(ADAMW, P) == 28 * 6


def test_plan_rows_and_cuts():
    rows, cuts = optimizer.plan([1, oc.CHUNK, oc.CHUNK + 1, 3])
    assert rows == [(0, 0), (1, 0), (2, 0), (2, 1), (3, 0)] and cuts == [(0, 4, 0, 5)]
    numels = [1 + (i % 3) * oc.CHUNK for i in range(2 * oc.MAX_TENSORS + 7)]
    rows, cuts = optimizer.plan(numels)
    assert [c[:2] for c in cuts] == [(0, oc.MAX_TENSORS), (oc.MAX_TENSORS, oc.MAX_TENSORS), (2 * oc.MAX_TENSORS, 7)]
    assert sum(c[3] for c in cuts) == len(rows) == sum(-(-n // oc.CHUNK) for n in numels)
    for first, count, first_block, n_blocks in cuts:                       # a cut's rows are exactly its tensors'
        assert {t for t, _ in rows[first_block:first_block + n_blocks]} == set(range(first, first + count))
    assert [t for t, _ in rows] == sorted(t for t, _ in rows)


class _Fake:
    """A parameter that claims to be what a test needs: the constructor looks at attributes only before it refuses."""
    requires_grad, layout = True, torch.strided

    def __init__(self, is_cuda, dtype, device="cuda:0", contiguous=True):
        self.is_cuda, self.dtype, self.device, self.contiguous = is_cuda, dtype, device, contiguous
        self.shape = (3, 5)

    def is_contiguous(self): return self.contiguous
    def stride(self): return (1, 3)


def test_construction_refusals():
    with pytest.raises(ValueError, match="dense fp32 CUDA parameters"):
        optimizer.FusedStepAdamW([torch.nn.Parameter(torch.zeros(3))])                  # a CPU parameter
    with pytest.raises(ValueError, match="dense fp32 CUDA parameters, got torch.float16"):
        optimizer.FusedStepAdamW([_Fake(True, torch.float16)])                          # an fp16 parameter on the device
    with pytest.raises(ValueError, match="dense fp32 CUDA parameters"):
        optimizer.FusedStepAdamW([torch.nn.Parameter(torch.zeros(3, dtype=torch.float16))])
    with pytest.raises(ValueError, match="on one device"):
        optimizer.FusedStepAdamW([_Fake(True, torch.float32, "cuda:0"), _Fake(True, torch.float32, "cuda:1")])
    with pytest.raises(ValueError, match="contiguous parameters"):
        optimizer.FusedStepAdamW([_Fake(True, torch.float32, contiguous=False)])
    with pytest.raises(ValueError, match="no parameter"):
        optimizer.FusedStepAdamW([torch.zeros(3)])
    import vivim_amd
    assert vivim_amd.FusedStepAdamW is optimizer.FusedStepAdamW


def test_make_optimizer_default_is_unchanged_and_the_env_opts_out(monkeypatch):
    from vivim_amd import train_step
    sig = inspect.signature(train_step.make_optimizer).parameters
    assert sig["fused_step"].default is False
    assert [n for n in sig][:6] == ["model", "lr", "weight_decay", "capturable", "fused", "lean"]
    monkeypatch.delenv("VIVIM_NO_FUSED_OPTIMIZER", raising=False)
    model = torch.nn.Linear(3, 2)
    stock = train_step.make_optimizer(model)
    assert type(stock) is torch.optim.AdamW and stock.defaults["lr"] == 1e-4 and stock.defaults["weight_decay"] == 1e-2
    with pytest.raises(ValueError, match="dense fp32 CUDA parameters"):                 # no quiet fall-back for a model it cannot take
        train_step.make_optimizer(model, fused_step=True)
    monkeypatch.setenv("VIVIM_NO_FUSED_OPTIMIZER", "1")
    assert type(train_step.make_optimizer(model, fused_step=True)) is torch.optim.AdamW


# ---- the restatement against the GPU test's bounds, on its inputs
@pytest.mark.parametrize("factor_case", oc.FACTORS)
@pytest.mark.parametrize("family", list(oc.P_FAMILIES))
@pytest.mark.parametrize("which", ["A", "B"])
def test_restated_update_meets_the_bounds(which, family, factor_case):
    p = torch.cat([t.reshape(-1) for t in oc.params_cpu(which, family, 5)])
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    worst = [0.0, 0.0, 0.0]
    for step in range(oc.STEPS):
        grads = oc.grads_cpu(which, step, 5)
        g = torch.cat([t.reshape(-1) for t in grads])
        inv_scale = 2.0 ** -16 if factor_case == "scaled" else 1.0
        if factor_case == "one":
            factor = torch.ones(())
        else:
            norm_true = oc.norm64(grads, inv_scale)
            max_norm = oc.CLIP_AT * norm_true if factor_case == "clip" else None
            norm = math.sqrt(float(oc.restate_sumsq(grads, inv_scale)))
            assert abs(norm - norm_true) <= oc.NORM_BOUND * norm_true
            clip, f = oc.factor64(norm, inv_scale, max_norm)
            factor = oc._f32(f)
            want_clip, want_f = oc.factor64(norm_true, inv_scale, max_norm)
            assert abs(float(oc._f32(clip)) - want_clip) <= 4 * oc.U * want_clip and abs(float(factor) - want_f) <= 4 * oc.U * want_f
        t = step + 1
        bc1, bc2s = oc.bias_corrections(t)
        (p64, m64, v64), bounds = oc.reference(p.double(), g.double(), m.double(), v.double(), float(factor), t)
        p, m, v = oc.restate_update(p, g, m, v, factor, bc1, bc2s)
        for i, (got, want, bound) in enumerate(zip((p, m, v), (p64, m64, v64), bounds)):
            worst[i] = max(worst[i], oc.worst(got.double(), want, bound))
    print("worst |error| / bound: p %.2f m %.2f v %.2f" % tuple(worst))
    assert max(worst) <= 1.0, worst


@pytest.mark.parametrize("scale", [1e-6, 1.0, 3e4])
@pytest.mark.parametrize("n", [1, 255, oc.CHUNK + 1, 1000003])
def test_restated_norm_meets_the_bound(n, scale):
    """The kernel's chain of 16 and the longest the bound is written for, 256."""
    g = [torch.randn(n, generator=torch.Generator().manual_seed(n)) * scale]
    want = oc.norm64(g)
    for iters in (oc.CHUNK // (oc.THREADS * oc.VEC), 64):
        got = math.sqrt(float(oc.restate_sumsq(g, 1.0, iters)))
        print("n %d scale %g chain %d: relative error %.2e of %.2e" % (n, scale, 4 * iters, abs(got - want) / want, oc.NORM_BOUND))
        assert abs(got - want) <= oc.NORM_BOUND * want
