"""CPU: the token-major residual add + norm entry points (include/vivim_hip.h: vivim_token_add_norm_params) are declared, exported
and present without disturbing the binding's tables; every bad argument is refused on the host before any launch, with a text
that names it; tm_add_supported refuses what the kernels do not take; the backbone switch keeps parameters and, on CPU tensors,
results; the reference surface (mamba_ssm.ops.triton.layernorm) agrees with an fp64 restatement; and a torch fp32 restatement
of the kernels' arithmetic meets the bounds tests/test_gpu_add_norm_tm.py asserts, on that test's inputs."""
import copy
import ctypes
import inspect
import os
import re

import pytest
import torch

import add_norm_tm_cases as cases
from conftest import ROOT
from vivim_amd import _lib
from vivim_amd import layernorm as ln

FWD, BWD, QUERY = "vivim_token_add_norm_fwd", "vivim_token_add_norm_bwd", "vivim_token_add_norm_bwd_workspace_bytes"
OK, INVALID, UNSUPPORTED = 0, 1, 2
PTR = 1 << 20                                    # a non-null, 16-byte aligned address: no check may dereference it
STRIDES = ("branch_row_stride", "res_row_stride", "res_out_row_stride", "y_row_stride", "dy_row_stride", "dres_row_stride",
           "dres_in_row_stride", "dbranch_row_stride")
POINTERS = ("branch", "res", "scale", "weight", "bias", "res_out", "y", "mean", "rstd", "dy", "dres", "dres_in", "dbranch",
            "dweight", "dbias", "workspace")


def _params(rows=35, C=64, btype=_lib.F32, rtype=_lib.F32, rps=5):
    P = _lib.TokenAddNormParams()
    P.struct_bytes = ctypes.sizeof(_lib.TokenAddNormParams)
    P.rows, P.channels, P.rows_per_sample, P.btype, P.rtype, P.otype, P.eps = rows, C, rps, btype, rtype, btype, 1e-5
    for f in STRIDES:
        setattr(P, f, C)
    for f in POINTERS:
        setattr(P, f, PTR)
    return P


def _refused(name, P, code, message):
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
    for name in (FWD, BWD, QUERY):
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert "vivim_token_add_norm_params" in text
    assert getattr(L, FWD).argtypes == [ctypes.POINTER(_lib.TokenAddNormParams), ctypes.c_void_p]
    assert getattr(L, QUERY).argtypes == [ctypes.POINTER(_lib.TokenAddNormParams)] and getattr(L, QUERY).restype is ctypes.c_size_t


def test_the_tables_are_undisturbed():
    L = _lib.lib()
    assert L.vivim_abi_version() == 8
    assert len(_lib.STRUCTS) == 15 and _lib.TokenAddNormParams not in _lib.STRUCTS
    assert L.vivim_sizeof(15) == 0
    for name in (FWD, BWD):
        e = _lib.ENTRY_POINTS[name]
        assert e.struct is None and e.extra == (ctypes.POINTER(_lib.TokenAddNormParams),) and e.stream and e.restype is ctypes.c_int
    e = _lib.ENTRY_POINTS[QUERY]
    assert e.struct is None and e.extra == (ctypes.POINTER(_lib.TokenAddNormParams),) and not e.stream and e.restype is ctypes.c_size_t
    assert [f[0] for f in _lib.TokenLayerNormParams._fields_] == [
        "struct_bytes", "rows", "channels", "itype", "otype", "eps", "x_row_stride", "y_row_stride", "dy_row_stride",
        "dx_row_stride", "x", "weight", "bias", "y", "mean", "rstd", "dy", "dx", "dweight", "dbias", "workspace"]
    fields = [f[0] for f in _lib.TokenAddNormParams._fields_]
    assert fields[:10] == ["struct_bytes", "rows", "channels", "rows_per_sample", "btype", "rtype", "otype", "rms", "eps", "_pad0"]
    assert tuple(fields[10:18]) == STRIDES and tuple(fields[18:]) == POINTERS


def test_null_struct_and_struct_bytes():
    L = _lib.lib()
    size = ctypes.sizeof(_lib.TokenAddNormParams)
    for name in (FWD, BWD):
        assert getattr(L, name)(None, None) == INVALID and b"check failed" in L.vivim_last_error()
        for bad in (size - 1, size + 1, 0):
            P = _params()
            P.struct_bytes = bad
            _refused(name, P, INVALID, "struct_bytes = %d" % bad)


def test_sizes_type_tags_and_pairs():
    for name in (FWD, BWD):
        _refused(name, _params(C=0), INVALID, "channels = 0")
        _refused(name, _params(C=1025), UNSUPPORTED, "channels = 1025")
        _refused(name, _params(rows=0), INVALID, "rows = 0")
        _refused(name, _params(rows=-3), INVALID, "rows = -3")
        for field in ("btype", "rtype", "otype"):
            P = _params()
            setattr(P, field, 3)
            _refused(name, P, INVALID, "%s = 3" % field)
        for bt, rt in ((_lib.F32, _lib.F16), (_lib.F32, _lib.BF16), (_lib.F16, _lib.BF16), (_lib.BF16, _lib.F16)):
            _refused(name, _params(btype=bt, rtype=rt), UNSUPPORTED, "branch type %d with residual type %d" % (bt, rt))
        P = _params(btype=_lib.BF16, rtype=_lib.F32)
        P.otype = _lib.F32                                            # y is written in the branch's type
        _refused(name, P, UNSUPPORTED, "output type 0")
        P = _params()
        P.rms = 2
        _refused(name, P, INVALID, "rms = 2")
        _refused(name, _params(rps=0), INVALID, "rows_per_sample = 0")
        _refused(name, _params(rps=-5), INVALID, "rows_per_sample = -5")
        _refused(name, _params(rps=6), INVALID, "rows_per_sample = 6")    # 35 rows
        P = _params(rps=0)
        P.scale = None                                               # without a scale nobody reads rows_per_sample
        P.struct_bytes = 0
        _refused(name, P, INVALID, "struct_bytes = 0")


def test_forward_pointers_and_strides():
    for field in ("branch", "y"):
        P = _params()
        setattr(P, field, None)
        _refused(FWD, P, INVALID, "%s is NULL" % field)
    P = _params()
    P.res_out = None                                                 # a residual that is read is a sum that is stored
    _refused(FWD, P, INVALID, "res_out is NULL")
    P = _params()
    P.weight = P.y = P.res_out = None                                # the add alone needs res_out and nothing else
    _refused(FWD, P, INVALID, "res_out is NULL")
    for keep, msg in (("mean", "rstd = (nil)"), ("rstd", "mean = (nil)")):
        P = _params()
        setattr(P, "rstd" if keep == "mean" else "mean", None)
        _refused(FWD, P, INVALID, msg)
    for field in ("branch", "res", "res_out", "y"):
        P = _params()
        setattr(P, field + "_row_stride", 63)
        _refused(FWD, P, INVALID, "%s_row_stride = 63" % field)
    for field, bt, rt in (("branch", _lib.BF16, _lib.F32), ("y", _lib.F16, _lib.F32), ("res", _lib.BF16, _lib.BF16),
                          ("res_out", _lib.F16, _lib.F16)):
        P = _params(btype=bt, rtype=rt)
        setattr(P, field, PTR + 1)                                   # one byte off is not element-aligned
        _refused(FWD, P, INVALID, "%s = 0x100001 is not aligned" % field)
    P = _params()
    P.res = PTR + 2                                                  # f32 on a 2-byte boundary
    _refused(FWD, P, INVALID, "res = 0x100002 is not aligned")
    for field in ("scale", "weight", "bias", "mean", "rstd"):
        P = _params()
        setattr(P, field, PTR + 2)
        _refused(FWD, P, INVALID, "%s = 0x100002 is not aligned" % field)


def test_backward_pointers_workspace_and_strides():
    for field in ("res_out", "mean", "rstd"):
        P = _params()
        setattr(P, field, None)
        _refused(BWD, P, INVALID, "%s is NULL" % field)
    P = _params()
    P.dy = P.dres = None
    _refused(BWD, P, INVALID, "dy and dres are both NULL")
    P = _params()
    P.weight = None                                                  # the add's backward alone has no dy
    _refused(BWD, P, INVALID, "without weight")
    for keep in ("dweight", "dbias"):
        P = _params()
        P.workspace = None
        setattr(P, "dbias" if keep == "dweight" else "dweight", None)
        _refused(BWD, P, INVALID, "need the workspace")
    for field in ("res_out", "dy", "dres", "dres_in", "dbranch"):
        P = _params()
        setattr(P, field + "_row_stride", 63)
        _refused(BWD, P, INVALID, "%s_row_stride = 63" % field)
    for field, bt, rt in (("dy", _lib.BF16, _lib.F32), ("dbranch", _lib.F16, _lib.F32), ("dres", _lib.BF16, _lib.BF16),
                          ("dres_in", _lib.F16, _lib.F16), ("res_out", _lib.BF16, _lib.BF16)):
        P = _params(btype=bt, rtype=rt)
        setattr(P, field, PTR + 1)
        _refused(BWD, P, INVALID, "%s = 0x100001 is not aligned" % field)
    for field in ("dweight", "dbias", "workspace", "scale", "mean"):
        P = _params()
        setattr(P, field, PTR + 2)
        _refused(BWD, P, INVALID, "%s = 0x100002 is not aligned" % field)


def test_workspace_formula_and_bytes():
    L = _lib.lib()
    for rows, C, slots in ((1, 64, 1), (37, 64, 10), (4133, 64, 1024), (4096, 8, 1024), (4092, 1000, 1023)):
        assert L.vivim_token_add_norm_bwd_workspace_bytes(ctypes.byref(_params(rows, C))) == slots * 2 * C * 4
        assert ln.tm_workspace_slots(rows) == slots              # the wrapper sizes the workspace by the header's formula
    assert L.vivim_token_add_norm_bwd_workspace_bytes(None) == 0
    assert L.vivim_token_add_norm_bwd_workspace_bytes(ctypes.byref(_params(C=1025))) == 0
    P = _params(100, 64, _lib.BF16, _lib.F32, rps=25)
    n = 100 * 64
    # forward: branch, res, res_out, y + mean, rstd + scale, weight, bias
    assert _lib.algorithmic_bytes(FWD, P) == n * (2 + 4 + 4 + 2) + 8 * 100 + 4 * 4 + 8 * 64
    # backward: res_out, dy, dres, dres_in, dbranch + mean, rstd + scale, weight, dweight, dbias
    assert _lib.algorithmic_bytes(BWD, P) == n * (4 + 2 + 4 + 4 + 2) + 8 * 100 + 4 * 4 + 12 * 64
    P.mean = P.rstd = P.scale = P.bias = None                    # the no-grad forward writes no statistics
    assert _lib.algorithmic_bytes(FWD, P) == n * (2 + 4 + 4 + 2) + 4 * 64
    P.res = None
    assert _lib.algorithmic_bytes(FWD, P) == n * (2 + 4 + 2) + 4 * 64
    P = _params(100, 64, _lib.BF16, _lib.F32, rps=25)
    P.weight = None                                              # the add alone: branch, res, res_out + scale | dres, dbranch + scale
    assert _lib.algorithmic_bytes(FWD, P) == n * (2 + 4 + 4) + 16
    P.dy = P.dres_in = None
    assert _lib.algorithmic_bytes(BWD, P) == n * (4 + 2) + 16
    P = _params(100, 64)
    P.dy = P.dweight = P.dbias = P.scale = P.dbranch = None       # dres alone: the saved row and the statistics are not read
    assert _lib.algorithmic_bytes(BWD, P) == n * (4 + 4) + 4 * 64


# ---- tm_add_supported ----------------------------------------------------------------------------------------------------------
class Fake:
    """A tensor's layout that claims to be on the GPU: the refusals need no device."""

    def __init__(self, t, cuda=True):
        self.t, self.is_cuda = t, cuda
        self.dtype, self.shape, self.device = t.dtype, t.shape, "cuda:0" if cuda else t.device

    def dim(self): return self.t.dim()
    def stride(self, d): return self.t.stride(d)
    def numel(self): return self.t.numel()
    def is_contiguous(self): return self.t.is_contiguous()


def test_tm_add_supported(monkeypatch):
    bf16 = torch.bfloat16
    res, branch, w = Fake(torch.randn(2, 5, 64)), Fake(torch.randn(2, 5, 64).to(bf16)), Fake(torch.ones(64))
    assert ln.tm_add_supported(res, branch, w, None) is True and ln.tm_add_supported(res, branch) is True
    assert ln.tm_add_rows(res, branch, w, Fake(torch.zeros(64))) == (10, 64, 64)
    assert ln.tm_add_rows(Fake(torch.randn(2, 5, 72)[..., :64]), branch) == (10, 72, 64)
    assert ln.tm_add_supported(torch.randn(2, 5, 64), torch.randn(2, 5, 64), torch.ones(64)) is False        # CPU tensors
    assert ln.tm_add_supported(Fake(torch.randn(2, 5, 64), cuda=False), branch, w) is False
    assert ln.tm_add_supported(res, Fake(torch.randn(2, 5, 64), cuda=False), w) is False
    assert ln.tm_add_supported(res, branch, Fake(torch.ones(64, dtype=bf16))) is False                       # a bf16 weight
    assert ln.tm_add_supported(res, branch, w, Fake(torch.zeros(64, dtype=bf16))) is False
    assert ln.tm_add_supported(Fake(torch.randn(2, 64, 5).transpose(1, 2)), branch, w) is False              # channel stride 5
    assert ln.tm_add_supported(res, Fake(torch.randn(2, 5, 128)[..., ::2]), w) is False                      # channel stride 2
    assert ln.tm_add_supported(Fake(torch.randn(2, 6, 64)[:, :5]), branch, w) is False                       # two row strides
    assert ln.tm_add_supported(res, Fake(torch.randn(2, 6, 64)[:, :5]), w) is False
    assert ln.tm_add_supported(res, Fake(torch.randn(2, 5, 32)), Fake(torch.ones(32))) is False              # a shape mismatch
    assert ln.tm_add_supported(res, Fake(torch.randn(10, 64)), w) is False
    assert ln.tm_add_supported(Fake(torch.randn(2, 5, 1025)), Fake(torch.randn(2, 5, 1025)), Fake(torch.ones(1025))) is False
    for bt, rt, ok in ((torch.float32, torch.float32, True), (torch.float16, torch.float16, True), (bf16, bf16, True),
                       (torch.float16, torch.float32, True), (bf16, torch.float32, True), (torch.float32, bf16, False),
                       (torch.float32, torch.float16, False), (torch.float16, bf16, False), (bf16, torch.float16, False),
                       (torch.float64, torch.float64, False)):
        assert ln.tm_add_supported(Fake(torch.zeros(3, 64, dtype=rt)), Fake(torch.zeros(3, 64, dtype=bt)), w) is ok, (bt, rt)
        assert ln.tm_add_pair_ok(bt, rt) is ok
    monkeypatch.setattr(_lib, "deterministic", lambda: True)                                                  # no atomics: still supported
    assert ln.tm_add_supported(res, branch, w, None) is True
    # what profiles/r10_add_norm_tm.txt gave: no stage shape of the bench where the call is at or below the composition in every run
    meta = torch.device("meta")
    assert not any(ln.tm_add_worthwhile(torch.empty(15, n, C, device=meta)) for n, C in ((4096, 64), (1024, 128), (256, 320), (64, 512)))
    with pytest.raises(ValueError, match="unsupported"):
        ln.add_layer_norm_tm(torch.randn(5, 64), torch.randn(5, 64), torch.ones(64), None)
    with pytest.raises(ValueError, match="unsupported"):
        ln.add_tm(torch.randn(5, 64), torch.randn(5, 64))


# ---- the switch ----------------------------------------------------------------------------------------------------------------
def _backbone():
    from transformers import SegformerConfig, SegformerForSemanticSegmentation
    cfg = SegformerConfig(num_channels=3, num_encoder_blocks=2, depths=[2, 1], sr_ratios=[2, 1], hidden_sizes=[16, 32],
                          patch_sizes=[7, 3], strides=[4, 2], num_attention_heads=[1, 2], mlp_ratios=[2, 2],
                          decoder_hidden_size=32, num_labels=3, drop_path_rate=0.1)
    torch.manual_seed(41)
    return SegformerForSemanticSegmentation(cfg)


def _blocks(backbone, **kw):
    from vivim_amd.vivim import mamba_block
    return mamba_block(backbone, 3, depths=[0, 0], dims=[16, 32], **kw)


def test_switch_exists_and_defaults_off():
    from vivim_amd import train_step, vivim
    for fn in (vivim.mamba_block.__init__, vivim.Vivim.__init__, train_step.build_model):
        assert inspect.signature(fn).parameters["fused_backbone_add_norm"].default is False
    assert _blocks(_backbone()).fused_backbone_add_norm is False


def test_switch_keeps_keys_and_parameter_identity():
    from vivim_amd.vivim import DropPath
    backbone = _backbone()
    before = {n: p for n, p in backbone.named_parameters()}
    stock_keys = list(_blocks(copy.deepcopy(backbone)).state_dict())
    block = _blocks(backbone, fused_backbone_add_norm=True)
    assert block.fused_backbone_add_norm is True and list(block.state_dict()) == stock_keys
    after = {n: p for n, p in backbone.named_parameters()}
    assert set(after) == set(before) and all(after[n] is before[n] for n in before)
    # the drop-path modules are the ones that can state their per-sample factor; the same rates
    paths = [m.drop_path for stage in block.downsample_layers.block for m in stage]
    assert len(paths) == 3 and all(isinstance(p, (DropPath, torch.nn.Identity)) for p in paths)
    assert sum(isinstance(p, DropPath) for p in paths) == 2 and all(type(m) is torch.nn.LayerNorm for m in block.modules()
                                                                    if isinstance(m, torch.nn.LayerNorm))


def test_switched_stage_on_the_cpu_is_the_stock_one_bit_for_bit(monkeypatch):
    from vivim_amd import vivim
    backbone = _backbone()
    stock = _blocks(copy.deepcopy(backbone)).eval()
    switched = _blocks(backbone, fused_backbone_add_norm=True).eval()
    stages = []
    real = vivim._run_stage
    monkeypatch.setattr(vivim, "_run_stage", lambda *a: (stages.append(len(a[0])), real(*a))[1])
    x = torch.randn(1, 2, 3, 32, 32, generator=torch.Generator().manual_seed(42))
    with torch.no_grad():
        a, b = stock(x), switched(x)
    assert stages == [2, 1]                                       # the switched model took the new route, the stock one did not
    assert len(a) == len(b) == 2 and all(torch.equal(u, v) for u, v in zip(a, b))
    with torch.autocast("cpu", dtype=torch.bfloat16), torch.no_grad():
        a, b = stock(x), switched(x)
    assert all(u.dtype == v.dtype and torch.equal(u, v) for u, v in zip(a, b))
    monkeypatch.setenv("VIVIM_NO_FUSED_LAYERNORM", "1")
    with torch.no_grad():
        c = switched(x)
    assert stages == [2, 1, 2, 1] and all(torch.equal(u, v) for u, v in zip(c, stock(x)))


def test_run_stage_handles_both_transformers_layouts_and_foreign_blocks():
    """layer_norm_1 / layer_norm_2 (transformers 4.x) run the same route; a block of neither form takes _run_block."""
    from vivim_amd import vivim
    blocks = _blocks(_backbone()).eval().downsample_layers.block[0]
    hs = torch.randn(2, 64, 16, generator=torch.Generator().manual_seed(43))

    class Old(torch.nn.Module):
        def __init__(self, blk):
            super().__init__()
            self.layer_norm_1, self.layer_norm_2 = blk.layernorm_before, blk.layernorm_after
            self.attention, self.mlp, self.drop_path = blk.attention, blk.mlp, blk.drop_path

    class Foreign(torch.nn.Module):
        def forward(self, hs, height, width):
            return (hs * 2,)

    with torch.no_grad():
        want = hs
        for blk in blocks:
            want = vivim._run_block(blk, want, 8, 8)
        assert torch.equal(vivim._run_stage(blocks, hs, 8, 8), want)
        assert torch.equal(vivim._run_stage([Old(b) for b in blocks], hs, 8, 8), want)
        mixed = vivim._run_stage([blocks[0], Foreign(), blocks[1]], hs, 8, 8)
        assert torch.equal(mixed, vivim._run_block(blocks[1], vivim._run_block(blocks[0], hs, 8, 8) * 2, 8, 8))


# ---- the reference surface -----------------------------------------------------------------------------------------------------
def _ln64(x, w, b, residual, eps, rms, residual_dtype):
    """fp64 restatement: the sum, rounded to the dtype it is stored in, then the norm of what was stored."""
    h = x.double() if residual is None else residual.double() + x.double()
    if residual_dtype is not None:
        h = h + (h.detach().to(residual_dtype).double() - h.detach())      # the stored value, gradients straight through
    return cases.norm64(h, w.double(), None if b is None else b.double(), eps, rms), h


def _row_err(got, want):
    C = want.shape[-1]
    g, r = got.detach().double().reshape(-1, C), want.detach().reshape(-1, C)
    return float(((g - r).norm(dim=1) / r.norm(dim=1).clamp_min(1e-30)).max())


def test_reference_surface_imports():
    import mamba_ssm.ops.triton.layernorm as surface
    from vivim_amd import layernorm_fn
    assert surface.layer_norm_fn is layernorm_fn.layer_norm_fn and surface.rms_norm_fn is layernorm_fn.rms_norm_fn
    assert surface.RMSNorm is layernorm_fn.RMSNorm
    sig = inspect.signature(surface.layer_norm_fn)
    assert list(sig.parameters) == ["x", "weight", "bias", "residual", "eps", "prenorm", "residual_in_fp32", "is_rms_norm"]
    assert [sig.parameters[k].default for k in ("residual", "eps", "prenorm", "residual_in_fp32", "is_rms_norm")] == \
        [None, 1e-6, False, False, False]
    sig = inspect.signature(surface.rms_norm_fn)
    assert list(sig.parameters) == ["x", "weight", "bias", "residual", "prenorm", "residual_in_fp32", "eps"]
    m = surface.RMSNorm(64)
    assert m.eps == 1e-5 and m.bias is None and "bias" in m._parameters and list(m.state_dict()) == ["weight"]
    assert torch.equal(m.weight, torch.ones(64))


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("with_residual", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("residual_in_fp32", [False, True], ids=["", "fp32"])
@pytest.mark.parametrize("prenorm", [False, True], ids=["", "prenorm"])
def test_reference_surface_on_the_cpu_against_fp64(prenorm, residual_in_fp32, with_residual, rms):
    from mamba_ssm.ops.triton.layernorm import layer_norm_fn, rms_norm_fn
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(3, 5, 64, generator=gen).requires_grad_(True)
    residual = torch.randn(3, 5, 64, generator=gen).requires_grad_(True) if with_residual else None
    w = (torch.randn(64, generator=gen) * 0.5 + 1).requires_grad_(True)
    b = (torch.randn(64, generator=gen) * 0.3).requires_grad_(True)
    dy, dres = torch.randn(3, 5, 64, generator=gen), torch.randn(3, 5, 64, generator=gen)
    if rms:
        out = rms_norm_fn(x, w, b, residual=residual, prenorm=prenorm, residual_in_fp32=residual_in_fp32, eps=1e-5)
    else:
        out = layer_norm_fn(x, w, b, residual=residual, eps=1e-5, prenorm=prenorm, residual_in_fp32=residual_in_fp32)
    assert isinstance(out, tuple) == prenorm
    y, res_out = out if prenorm else (out, None)
    assert y.dtype == x.dtype and y.shape == x.shape
    if prenorm:
        assert res_out.dtype == torch.float32 and res_out.shape == x.shape
        if not with_residual and not residual_in_fp32:
            assert res_out is x                                   # nothing was added and nothing was cast
    x64 = x.detach().double().requires_grad_(True)
    r64 = None if residual is None else residual.detach().double().requires_grad_(True)
    y64, h64 = _ln64(x64, w.detach(), b.detach(), r64, 1e-5, rms, torch.float32)
    torch.autograd.backward([y64] + ([h64] if prenorm else []), [dy.double()] + ([dres.double()] if prenorm else []))
    torch.autograd.backward([y] + ([res_out] if prenorm else []), [dy] + ([dres] if prenorm else []))
    assert _row_err(y, y64) < 2e-6 and _row_err(x.grad, x64.grad) < 1e-5
    if with_residual:
        assert _row_err(residual.grad, r64.grad) < 1e-5
        if prenorm:
            assert _row_err(res_out, h64) < 2e-6


def test_reference_surface_dtypes_and_rmsnorm_module():
    from mamba_ssm.ops.triton.layernorm import RMSNorm, layer_norm_fn, rms_norm_fn
    bf16 = torch.bfloat16
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(4, 64, generator=gen).to(bf16)
    residual = torch.randn(4, 64, generator=gen)
    w, b = torch.randn(64, generator=gen).to(bf16).requires_grad_(True), torch.zeros(64)       # a bf16 weight is cast with .float()
    y, r = layer_norm_fn(x, w, b, residual=residual, prenorm=True)
    assert y.dtype == bf16 and r.dtype == torch.float32                                       # the residual's dtype
    y.float().sum().backward()
    assert w.grad.dtype == bf16                                                               # autograd casts the gradient back
    y, r = layer_norm_fn(x, w, b, residual=residual.to(bf16), prenorm=True)
    assert y.dtype == bf16 and r.dtype == bf16
    y, r = layer_norm_fn(x, w, b, prenorm=True, residual_in_fp32=True)
    assert y.dtype == bf16 and r.dtype == torch.float32 and torch.equal(r, x.float())
    y, r = rms_norm_fn(x, w, None, prenorm=True)
    assert r is x
    y64, _ = _ln64(x, w.detach(), None, None, 1e-6, True, None)
    assert _row_err(y, y64) < 4e-3
    m = RMSNorm(64, eps=1e-5)
    with torch.no_grad():
        m.weight.copy_(torch.randn(64, generator=gen))
    xf = torch.randn(3, 5, 64, generator=gen)
    y64, _ = _ln64(xf, m.weight.detach(), None, None, 1e-5, True, None)
    assert _row_err(m(xf), y64) < 2e-6
    y2, r2 = m(xf, residual=xf, prenorm=True)
    assert torch.equal(r2, xf + xf)
    big = torch.randn(2, 2048, generator=gen)                                                  # C > 1024: the same definition
    y64, _ = _ln64(big, torch.ones(2048), None, None, 1e-6, False, None)
    assert _row_err(layer_norm_fn(big, torch.ones(2048), None), y64) < 2e-6


# ---- the definition meets the GPU test's bounds ----------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(cases.FAMILIES))
@pytest.mark.parametrize("btype,rtype", cases.PAIRS, ids=lambda d: cases.name(d))
def test_the_kernels_arithmetic_in_torch_fp32_meets_the_gpu_bounds(btype, rtype, family):
    """A bound must never be one the definition itself misses: the restated arithmetic (cases.emulate), on the inputs of
    tests/test_gpu_add_norm_tm.py, passes the same cases.ratios < 1."""
    worst = {}
    for layout, shape in cases.SHAPES + ([cases.BIG] if btype == rtype == cases.F32 else []):
        inp = cases.inputs(layout, shape, family, btype, rtype, seed=sum(shape) + 7 * len(shape))
        for rms, bias, eps, kind in cases.COMBOS:
            scale = cases.scale_of(kind, shape[0])
            b = inp["b"] if bias else None
            got = cases.emulate(inp["res"], inp["branch"], scale, inp["w"], b, inp["dy"], inp["dres"], eps, rms)
            ref = cases.reference(got["res_new"], inp["res"], inp["branch"], scale, inp["w"], b, inp["dy"], inp["dres"], eps, rms)
            r = cases.ratios(got, ref, scale, btype, rtype, family, eps, rms)
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert all(v < 1.0 for v in r.values()), (layout, shape, rms, bias, eps, kind, r)
    print(f"{cases.name(btype)}/{cases.name(rtype)} {family}: worst err / bound " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
