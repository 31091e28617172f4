"""CPU: the master-weight form of the fused clip + AdamW step (include/vivim_hip.h: vivim_opt_mw_params).  Its entry points are
declared, exported and present beside the fp32 ones; every bad argument is refused on the host before any launch; the
constructor's default is what it was; the tables sort by class and no call mixes classes; `lower_params` changes exactly the
intended parameters, `raise_params` restores every bit, and a lowered model under bf16 autocast computes the stock model's outputs
and gradients bit for bit; the kernel's two narrowing conversions, restated, are torch's cast on the families the GPU test runs
(master_weights_cases.py); and the guards of make_optimizer / train_step / eval_step / dp.wrap hold."""
import copy
import ctypes
import inspect
import os
import re

import pytest
import torch

import fused_optimizer_cases as oc
import master_weights_cases as mc
from conftest import ROOT
from vivim_amd import _lib, optimizer

STATS, ADAMW = "vivim_opt_grad_stats_mw", "vivim_opt_adamw_mw"
INVALID = 1
PTR = 1 << 20                                    # a non-null, 16-byte aligned address: no check may dereference it


def _params(count=3, numels=(5, 4097, 1), total_blocks=4, dtype=_lib.BF16):
    """A call both entry points accept up to the launch: the host arrays are real, the device pointers are not memory."""
    P = _lib.OptMwParams()
    P.struct_bytes = ctypes.sizeof(_lib.OptMwParams)
    P.count, P.first_tensor, P.first_block, P.n_blocks, P.total_blocks = count, 0, 0, total_blocks, total_blocks
    P.scaled, P.has_max_norm, P.max_norm = 1, 1, 1.0
    P.lr, P.beta1, P.beta2, P.eps, P.weight_decay = 1e-3, 0.9, 0.999, 1e-8, 1e-2
    n = max(count, 1)
    grads = (_lib.vp * n)(*([PTR] * n))
    numel = (_lib.i64 * n)(*(list(numels) + [1] * n)[:n])
    P.grads, P.numel = ctypes.cast(grads, ctypes.POINTER(_lib.vp)), ctypes.cast(numel, ctypes.POINTER(_lib.i64))
    P._keep = (grads, numel)
    for f in ("params", "exp_avg", "exp_avg_sq", "block_map", "state", "workspace", "masters"):
        setattr(P, f, PTR)
    P.workspace_bytes = 8 * total_blocks
    P.dtype = dtype
    return P


def _refused(name, P, message):
    L = _lib.lib()
    assert getattr(L, name)(ctypes.byref(P), None) == INVALID, L.vivim_last_error()
    direct = L.vivim_last_error().decode()
    assert message in direct, direct
    with pytest.raises(RuntimeError) as info:
        _lib.call(name, P, 0)
    assert str(info.value) == direct


def test_symbols_declared_exported_and_present():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vivim_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vivim_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    assert L.vivim_abi_version() == 8
    for name in (STATS, ADAMW):
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes == [ctypes.POINTER(_lib.OptMwParams), ctypes.c_void_p]
        e = _lib.ENTRY_POINTS[name]
        assert e.struct is None and e.extra == (ctypes.POINTER(_lib.OptMwParams),) and e.stream and e.restype is ctypes.c_int
    assert "vivim_opt_mw_params" in text and _lib.OptMwParams not in _lib.STRUCTS
    # the struct: vivim_opt_step_params field for field, then masters, dtype and padding to 8 bytes
    step = ctypes.sizeof(_lib.OptStepParams)
    assert [f[0] for f in _lib.OptMwParams._fields_][:-3] == [f[0] for f in _lib.OptStepParams._fields_]
    assert _lib.OptMwParams.masters.offset == step and _lib.OptMwParams.dtype.offset == step + 8
    assert ctypes.sizeof(_lib.OptMwParams) == step + 16
    body = re.search(r"typedef struct \{([^}]*)\} vivim_opt_mw_params;", text).group(1)
    fields = re.findall(r"(\w+)\s*(?:,|;)", body)
    assert fields == [f[0] for f in _lib.OptMwParams._fields_]
    # the library agrees on the size: a call with it gets past the struct_bytes check, to the next one
    P = _params()
    P.dtype = 0
    _refused(STATS, P, "dtype = 0")


def test_entry_points_refuse_bad_arguments():
    L = _lib.lib()
    size = ctypes.sizeof(_lib.OptMwParams)
    for name in (STATS, ADAMW):
        assert getattr(L, name)(None, None) == INVALID and b"check failed" in L.vivim_last_error()
        for bad in (size - 8, size + 8, ctypes.sizeof(_lib.OptStepParams), 0):
            P = _params()
            P.struct_bytes = bad
            _refused(name, P, "struct_bytes = %d, this library's vivim_opt_mw_params has %d" % (bad, size))
        for bad in (0, _lib.OPT_MAX_TENSORS + 1):
            assert _lib.OPT_MAX_TENSORS + 1 == 249
            P = _params()
            P.count = bad
            _refused(name, P, "count = %d" % bad)
        for bad in (0, 3, -1):
            _refused(name, _params(dtype=bad), "dtype = %d" % bad)
        for field in ("state", "block_map"):
            P = _params()
            setattr(P, field, None)
            _refused(name, P, "check failed")
        for field, typ in (("grads", _lib.vp), ("numel", _lib.i64)):
            P = _params()
            setattr(P, field, ctypes.POINTER(typ)())
            _refused(name, P, "check failed")
        _refused(name, _params(numels=(5, 0, 1)), "numel[1] = 0")
        P = _params()
        P.first_block, P.n_blocks = 3, 2
        _refused(name, P, "map rows 3 .. 3 + 2 of 4")
    for field in ("masters", "params", "exp_avg", "exp_avg_sq"):
        P = _params()
        setattr(P, field, None)
        _refused(ADAMW, P, "check failed")
    P = _params()
    P.workspace_bytes = 31
    _refused(STATS, P, "workspace of 31 bytes at 0x100000: need a 8-byte aligned one of vivim_opt_step_workspace_bytes() = 32")
    P = _params()
    P.workspace = None
    _refused(STATS, P, "workspace of 32 bytes at (nil)")
    P = _params()
    P.lr = -1e-3
    _refused(ADAMW, P, "lr = -0.001")
    P = _params()
    P.beta1 = 1.0
    _refused(ADAMW, P, "betas = ")
    P = _params()
    P._keep[0][1] = PTR + 1                                               # a 16-bit gradient is at least 2-byte aligned
    _refused(STATS, P, "check failed")


def test_bytes_moved_estimate():
    P = _params()                                                          # 5 + 4097 + 1 elements, 4 map rows
    assert _lib.algorithmic_bytes(STATS, P) == 2 * 4103 + 8 * 4
    assert _lib.algorithmic_bytes(ADAMW, P) == (2 + 12 + 12 + 2) * 4103 == 28 * 4103    # the fp32 step's bytes
    P._keep[0][1] = None
    assert _lib.algorithmic_bytes(STATS, P) == 2 * 6 + 8 * 4 and _lib.algorithmic_bytes(ADAMW, P) == 28 * 6


class _Fake:
    requires_grad, layout = True, torch.strided

    def __init__(self, is_cuda, dtype, device="cuda:0"):
        self.is_cuda, self.dtype, self.device, self.shape = is_cuda, dtype, device, (3, 5)

    def is_contiguous(self): return True


def test_constructor_default_and_refusals():
    sig = inspect.signature(optimizer.FusedStepAdamW.__init__).parameters
    assert sig["master_weights"].default is False
    with pytest.raises(ValueError, match="dense fp32 CUDA parameters, got torch.float16"):      # today's text
        optimizer.FusedStepAdamW([_Fake(True, torch.float16)])
    with pytest.raises(ValueError, match="dense fp32 CUDA parameters, got torch.bfloat16"):
        optimizer.FusedStepAdamW([_Fake(True, torch.bfloat16)], master_weights=False)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match=r"master_weights=True\) takes dense fp32, fp16 or bf16 CUDA parameters, got .* on cpu"):
            optimizer.FusedStepAdamW([torch.nn.Parameter(torch.zeros(3, dtype=dtype))], master_weights=True)
    with pytest.raises(ValueError, match="fp32, fp16 or bf16 CUDA parameters, got torch.float64"):
        optimizer.FusedStepAdamW([_Fake(True, torch.float64)], master_weights=True)
    with pytest.raises(ValueError, match="on one device"):
        optimizer.FusedStepAdamW([_Fake(True, torch.float16, "cuda:0"), _Fake(True, torch.float32, "cuda:1")], master_weights=True)
    import vivim_amd
    assert vivim_amd.lower_params is optimizer.lower_params and vivim_amd.raise_params is optimizer.raise_params


def test_tables_sort_by_class_and_no_cut_mixes_classes():
    dtypes = [(torch.float32, torch.bfloat16, torch.float16)[i % 3] for i in range(600)]
    order = optimizer.table_order(dtypes)
    assert sorted(order) == list(range(600))
    assert [dtypes[i] for i in order] == [torch.float32] * 200 + [torch.float16] * 200 + [torch.bfloat16] * 200
    for cls in range(3):                                                   # inside a class the list's order is kept
        part = order[200 * cls:200 * (cls + 1)]
        assert part == sorted(part)
    classes = [optimizer.CLASSES.index(dtypes[i]) for i in order]
    assert (_lib.F32, _lib.F16, _lib.BF16) == (0, 1, 2) and optimizer.CLASSES == (torch.float32, torch.float16, torch.bfloat16)
    numels = [1 + (i % 3) * oc.CHUNK for i in order]
    rows, cuts = optimizer.plan(numels, classes)
    assert [c[:2] for c in cuts] == [(0, 200), (200, 200), (400, 200)]
    # 300 per class: every class needs two calls, and the cap holds
    dtypes = [(torch.float32, torch.bfloat16, torch.float16)[i % 3] for i in range(900)]
    order = optimizer.table_order(dtypes)
    classes = [optimizer.CLASSES.index(dtypes[i]) for i in order]
    numels = [1 + (i % 5) * 1000 for i in order]
    rows, cuts = optimizer.plan(numels, classes)
    assert [c[:2] for c in cuts] == [(0, 248), (248, 52), (300, 248), (548, 52), (600, 248), (848, 52)]
    covered = []
    for first, count, first_block, n_blocks in cuts:
        assert 1 <= count <= oc.MAX_TENSORS == 248
        assert len({classes[t] for t in range(first, first + count)}) == 1
        assert {t for t, _ in rows[first_block:first_block + n_blocks]} == set(range(first, first + count))
        covered.extend(range(first, first + count))
    assert covered == list(range(900)) and sum(c[3] for c in cuts) == len(rows) == sum(-(-n // oc.CHUNK) for n in numels)
    assert optimizer.plan(numels) == optimizer.plan(numels, [0] * 900)     # one class: the cuts of the fp32 route


# ---- lowering a model ---------------------------------------------------------------------------------------------------------
class MambaLayer(torch.nn.Module):
    """Stands in for vivim.MambaLayer, which lower_params recognises by its class name: everything below it stays fp32."""

    def __init__(self):
        super().__init__()
        self.norm = torch.nn.LayerNorm(32)
        self.proj = torch.nn.Linear(32, 32)

    def forward(self, x):
        return x + self.proj(self.norm(x))


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from transformers import SegformerConfig, SegformerForSemanticSegmentation
        from vivim_amd.vivim import mamba_block
        cfg = SegformerConfig(num_channels=3, num_encoder_blocks=2, depths=[2, 1], sr_ratios=[2, 1], hidden_sizes=[16, 32],
                              patch_sizes=[7, 3], strides=[4, 2], num_attention_heads=[1, 2], mlp_ratios=[2, 2],
                              decoder_hidden_size=32, num_labels=3)
        torch.manual_seed(41)
        self.encoder = mamba_block(SegformerForSemanticSegmentation(cfg), 3, depths=[0, 0], dims=[16, 32],
                                   fast_backbone_dwconv=True, fast_backbone_layernorm=True)
        self.mixer = MambaLayer()
        self.bn = torch.nn.BatchNorm2d(32)
        self.out = torch.nn.Conv2d(32, 3, kernel_size=1)

    def forward(self, x):
        feat = self.encoder(x)[-1]                                        # (B * nf, 32, H, W)
        feat = self.mixer(feat.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
        return self.out(self.bn(feat))


def _expected_lowered(model):
    """Names of the parameters lower_params is specified to lower, derived here from the module tree."""
    from vivim_amd.vivim import _TokenDWConv2d
    keep = set()
    for name, m in model.named_modules():
        if isinstance(m, (MambaLayer, _TokenDWConv2d)):
            keep.update(name + "." + n for n, _ in m.named_parameters())
    want = set()
    for name, m in model.named_modules():
        if type(m) in (torch.nn.Linear, torch.nn.Conv2d):
            want.update(name + "." + n for n, _ in m.named_parameters(recurse=False))
    return want - keep


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_lower_params_and_raise_params(dtype):
    from vivim_amd.vivim import _BackboneLayerNorm, _TokenDWConv2d
    model = _Tiny()
    start = {n: p.detach().clone() for n, p in model.named_parameters()}
    keys = list(model.state_dict())
    want = _expected_lowered(model)
    assert any(isinstance(m, _TokenDWConv2d) for m in model.modules()) and any(isinstance(m, _BackboneLayerNorm) for m in model.modules())
    assert "out.weight" in want and "out.bias" in want and "mixer.proj.weight" not in want and len(want) > 20
    assert not any(".dwconv.dwconv." in n for n in want) and any(".dwconv.dwconv." in n for n in start)
    lowered = optimizer.lower_params(model, dtype)
    assert model._vivim_param_dtype == dtype
    names = {id(p): n for n, p in model.named_parameters()}
    assert {names[id(p)] for p in lowered} == want and len(lowered) == len(want)
    for n, p in model.named_parameters():
        assert p.dtype == (dtype if n in want else torch.float32), n
        if n in want:
            assert p.master_fp32.dtype == torch.float32 and torch.equal(p.master_fp32, start[n])       # the original bits
            assert torch.equal(mc.bits16(p.detach()), mc.bits16(start[n].to(dtype)))                  # autocast's cast of them
        else:
            assert not hasattr(p, "master_fp32") and torch.equal(p, start[n])
    for m in model.modules():                                              # every norm is fp32
        if isinstance(m, (torch.nn.LayerNorm, torch.nn.BatchNorm2d)):
            assert all(p.dtype == torch.float32 for p in m.parameters())
    assert list(model.state_dict()) == keys
    with pytest.raises(ValueError, match="already stored"):
        optimizer.lower_params(model, dtype)
    raised = optimizer.raise_params(model)
    assert {names[id(p)] for p in raised} == want and model._vivim_param_dtype is None
    for n, p in model.named_parameters():
        assert p.dtype == torch.float32 and torch.equal(p, start[n]) and not hasattr(p, "master_fp32"), n
    assert list(model.state_dict()) == keys
    with pytest.raises(ValueError, match="float16 or torch.bfloat16"):
        optimizer.lower_params(model, torch.float32)


def test_raise_params_takes_the_optimizers_masters():
    model = _Tiny()
    lowered = optimizer.lower_params(model, torch.bfloat16)

    class Opt:                                                            # what raise_params reads of a FusedStepAdamW
        params = lowered[:3]
        masters = [p.master_fp32 + 1.0 for p in lowered[:3]]
    want = [w.clone() for w in Opt.masters] + [p.master_fp32.clone() for p in lowered[3:]]
    optimizer.raise_params(model, Opt)
    assert all(p.dtype == torch.float32 and torch.equal(p, w) for p, w in zip(lowered, want))


def test_a_lowered_model_under_bf16_autocast_is_the_stock_model_bit_for_bit():
    stock = _Tiny().train()
    low = copy.deepcopy(stock)
    lowered = optimizer.lower_params(low, torch.bfloat16)
    x = torch.randn(1, 2, 3, 32, 32, generator=torch.Generator().manual_seed(42))
    outs = []
    for model in (stock, low):
        with torch.autocast("cpu", dtype=torch.bfloat16):
            y = model(x)
        y.float().square().mean().backward()
        outs.append(y)
    assert outs[0].dtype == outs[1].dtype and torch.equal(outs[0], outs[1])
    ids = {id(p) for p in lowered}
    checked = 0
    for (n, a), (_, b) in zip(stock.named_parameters(), low.named_parameters()):
        if a.grad is None:
            assert b.grad is None, n
            continue
        assert a.grad.dtype == torch.float32 and b.grad.dtype == b.dtype == (torch.bfloat16 if id(b) in ids else torch.float32), n
        assert torch.equal(a.grad, b.grad.float()), n                      # widened: bit-equal
        checked += id(b) in ids
    assert checked > 20


# ---- the rounding the kernel performs, restated ---------------------------------------------------------------------------------
def _masters_after_a_step(p):
    """master' of one restated fp32 step (fused_optimizer_cases.restate_update) from p with a gradient of its own scale."""
    g = torch.randn(p.shape, generator=torch.Generator().manual_seed(8)) * p.abs().mean()
    bc1, bc2s = oc.bias_corrections(1)
    return oc.restate_update(p, g, torch.zeros_like(p), torch.zeros_like(p), torch.ones(()), bc1, bc2s)[0]


@pytest.mark.parametrize("dtype", mc.DTYPES)
def test_restated_narrowing_is_torchs_cast(dtype):
    """master' -> p16 on the families of fused_optimizer_cases and on the two rounding families: the restated conversions agree
    with `.to(dtype)` in every bit, so the GPU test's expectation (p16 == master.to(dtype)) is reachable for these inputs."""
    restated = mc.narrow_f16_restated if dtype == torch.float16 else mc.narrow_bf16_restated
    inputs = {}
    for which in ("A", "B"):
        for fam in oc.P_FAMILIES:
            p = torch.cat([t.reshape(-1) for t in oc.params_cpu(which, fam, 5)])
            inputs["%s %s" % (which, fam)] = _masters_after_a_step(p)
    for fam in mc.FAMILIES:
        inputs[fam] = mc.family(fam)
    inputs["specials"] = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 1.0, 2.0 ** -149, -2.0 ** -126, 3.3e38, 1.00390625, 1.01171875])
    for name, x in inputs.items():
        want = mc.bits16(x.to(dtype))
        assert torch.equal(restated(x), want), (name, dtype)
    # what the families are there for
    sub, over = mc.family("subnormal").to(dtype), mc.family("overflow").to(dtype)
    if dtype == torch.float16:
        assert bool((sub.float().abs() < 2.0 ** -14).all()) and int((sub != 0).sum()) > 4000       # subnormal results, not flushed
        ties = sub[:64].float().abs() * 2.0 ** 24                          # halfway k + 1/2: to the even neighbour
        assert torch.equal(ties, torch.tensor([float(k + (k % 2)) for k in range(1, 65)]))
        assert over[:4].abs().tolist() == [65504.0, 65504.0, float("inf"), float("inf")]
        assert 0 < int(torch.isinf(over).sum()) < over.numel() and not bool(torch.isnan(over).any())
    else:
        assert bool(torch.isfinite(sub).all()) and bool(torch.isfinite(over).all()) and int((sub != 0).sum()) == sub.numel()
        assert bool(torch.isnan(torch.tensor([float("nan")]).to(dtype)).all())
        assert mc.narrow_bf16_restated(torch.tensor([float("nan")])).tolist() == [0x7FC0]


# ---- guards -------------------------------------------------------------------------------------------------------------------
def test_make_optimizer_needs_both_switches_for_a_lowered_model(monkeypatch):
    from vivim_amd import train_step
    sig = inspect.signature(train_step.make_optimizer).parameters
    assert sig["master_weights"].default is False and sig["fused_step"].default is False
    assert inspect.signature(train_step.build_model).parameters["low_precision_params"].default is None
    monkeypatch.delenv("VIVIM_NO_FUSED_OPTIMIZER", raising=False)
    model = torch.nn.Sequential(torch.nn.Linear(3, 2))
    optimizer.lower_params(model, torch.bfloat16)
    for kw in ({}, {"fused_step": True}, {"master_weights": True}, {"lean": False}):
        with pytest.raises(ValueError, match="raise_params"):
            train_step.make_optimizer(model, **kw)
    with pytest.raises(ValueError, match=r"master_weights=True\) takes dense fp32, fp16 or bf16 CUDA parameters"):
        train_step.make_optimizer(model, fused_step=True, master_weights=True)      # both switches: the constructor's own refusal (CPU)
    monkeypatch.setenv("VIVIM_NO_FUSED_OPTIMIZER", "1")
    with pytest.raises(ValueError, match="raise_params"):                            # the env switch is no quiet fall-back either
        train_step.make_optimizer(model, fused_step=True, master_weights=True)
    optimizer.raise_params(model)
    assert type(train_step.make_optimizer(model)) is torch.optim.AdamW and model[0].weight.dtype == torch.float32


def test_autocast_dtype_guard_and_dp_refusal(monkeypatch):
    from vivim_amd import dp, train_step
    model = torch.nn.Sequential(torch.nn.Linear(3, 2))
    for amp in (torch.float32, torch.float16, torch.bfloat16):
        optimizer.check_autocast_dtype(model, amp)                         # a stock model: any dtype
    optimizer.lower_params(model, torch.bfloat16)
    optimizer.check_autocast_dtype(model, torch.bfloat16)
    clip, onehot = torch.zeros(1, 1, 3, 8, 8), torch.zeros(1, 1, 3, 8, 8)
    for amp in (torch.float16, torch.float32):
        with pytest.raises(ValueError, match="stored in torch.bfloat16"):
            optimizer.check_autocast_dtype(model, amp)
        with pytest.raises(ValueError, match="stored in torch.bfloat16.*raise_params"):   # before anything else happens
            train_step.train_step(model, None, clip, onehot, 3, amp)
        with pytest.raises(ValueError, match="stored in torch.bfloat16.*raise_params"):
            train_step.eval_step(model, clip, onehot, 3, amp_dtype=amp)
    # the data-parallel wrapper: the identity without a process group, as before; with one (a rehearsal world of one rank on
    # gloo) it refuses the lowered model and wraps the raised one
    import torch.distributed as dist
    assert dp.wrap(model) is model
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        monkeypatch.setattr(dp, "_REHEARSE", True)
        with pytest.raises(ValueError, match="stored in torch.bfloat16.*16-bit gradients across ranks.*raise_params"):
            dp.wrap(model)
        optimizer.raise_params(model)
        assert isinstance(dp.wrap(model), torch.nn.parallel.DistributedDataParallel)
    finally:
        dist.destroy_process_group()
