"""CPU: the token-major LayerNorm's entry points (include/vivim_hip.h: vivim_token_layernorm_params) are declared, exported and
present without disturbing the binding's tables; every bad argument is refused on the host before any launch, with its text;
tm_supported refuses what the kernels do not take; and the backbone swap keeps parameters and, on CPU tensors, results."""
import copy
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT
from vivim_amd import _lib
from vivim_amd import layernorm as ln

FWD, BWD, QUERY = "vivim_token_layernorm_fwd", "vivim_token_layernorm_bwd", "vivim_token_layernorm_bwd_workspace_bytes"
OK, INVALID, UNSUPPORTED = 0, 1, 2
PTR = 1 << 20                                    # a non-null, 16-byte aligned address: no check may dereference it


def _params(rows=37, C=64, itype=_lib.F32, otype=_lib.F32):
    P = _lib.TokenLayerNormParams()
    P.struct_bytes = ctypes.sizeof(_lib.TokenLayerNormParams)
    P.rows, P.channels, P.itype, P.otype, P.eps = rows, C, itype, otype, 1e-5
    P.x_row_stride = P.y_row_stride = P.dy_row_stride = P.dx_row_stride = C
    for f in ("x", "weight", "bias", "y", "mean", "rstd", "dy", "dx", "dweight", "dbias", "workspace"):
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
    assert "vivim_token_layernorm_params" in text
    assert getattr(L, FWD).argtypes == [ctypes.POINTER(_lib.TokenLayerNormParams), ctypes.c_void_p]
    assert getattr(L, QUERY).argtypes == [ctypes.POINTER(_lib.TokenLayerNormParams)] and getattr(L, QUERY).restype is ctypes.c_size_t


def test_the_tables_are_undisturbed():
    L = _lib.lib()
    assert L.vivim_abi_version() == 8
    assert len(_lib.STRUCTS) == 15 and _lib.TokenLayerNormParams not in _lib.STRUCTS
    assert L.vivim_sizeof(15) == 0
    for name in (FWD, BWD):
        e = _lib.ENTRY_POINTS[name]
        assert e.struct is None and e.extra == (ctypes.POINTER(_lib.TokenLayerNormParams),) and e.stream and e.restype is ctypes.c_int
    e = _lib.ENTRY_POINTS[QUERY]
    assert e.struct is None and e.extra == (ctypes.POINTER(_lib.TokenLayerNormParams),) and not e.stream and e.restype is ctypes.c_size_t
    assert [f[0] for f in _lib.TokenLayerNormParams._fields_] == [
        "struct_bytes", "rows", "channels", "itype", "otype", "eps", "x_row_stride", "y_row_stride", "dy_row_stride",
        "dx_row_stride", "x", "weight", "bias", "y", "mean", "rstd", "dy", "dx", "dweight", "dbias", "workspace"]


def test_null_struct_and_struct_bytes():
    L = _lib.lib()
    size = ctypes.sizeof(_lib.TokenLayerNormParams)
    for name in (FWD, BWD):
        assert getattr(L, name)(None, None) == INVALID and b"check failed" in L.vivim_last_error()
        for bad in (size - 1, size + 1, 0):
            P = _params()
            P.struct_bytes = bad
            _refused(name, P, INVALID, "struct_bytes = %d" % bad)


def test_channel_counts_and_type_pairs():
    for name in (FWD, BWD):
        _refused(name, _params(C=0), INVALID, "channels = 0")
        _refused(name, _params(C=1025), UNSUPPORTED, "channels = 1025")
        for it, ot in ((_lib.F16, _lib.BF16), (_lib.BF16, _lib.F16)):
            _refused(name, _params(itype=it, otype=ot), UNSUPPORTED, "input type %d with output type %d" % (it, ot))
        for field in ("itype", "otype"):
            P = _params()
            setattr(P, field, 3)
            _refused(name, P, INVALID, "check failed")
        _refused(name, _params(rows=0), INVALID, "check failed")


def test_null_pointers_workspace_and_strides():
    for field in ("x", "y", "weight"):
        P = _params()
        setattr(P, field, None)
        _refused(FWD, P, INVALID, "check failed")
    P = _params()
    P.rstd = None                                                # mean without rstd
    _refused(FWD, P, INVALID, "check failed")
    for field in ("x", "dy", "dx", "mean", "rstd", "weight"):
        P = _params()
        setattr(P, field, None)
        _refused(BWD, P, INVALID, "check failed")
    for keep in ("dweight", "dbias"):
        P = _params()
        P.workspace = None
        setattr(P, "dbias" if keep == "dweight" else "dweight", None)
        _refused(BWD, P, INVALID, "need the workspace")
    P = _params()
    P.x_row_stride = 63
    _refused(FWD, P, INVALID, "x_row_stride = 63")
    _refused(BWD, P, INVALID, "x_row_stride = 63")
    P = _params()
    P.y_row_stride = 63
    _refused(FWD, P, INVALID, "y_row_stride = 63")
    for field in ("dy_row_stride", "dx_row_stride"):
        P = _params()
        setattr(P, field, 63)
        _refused(BWD, P, INVALID, "%s = 63" % field)
    P = _params(itype=_lib.BF16, otype=_lib.BF16)               # one byte off is not element-aligned
    P.x = PTR + 1
    _refused(FWD, P, INVALID, "check failed")


def test_workspace_formula_and_bytes():
    L = _lib.lib()
    for rows, C, slots in ((1, 64, 1), (37, 64, 10), (4133, 64, 1024), (4096, 8, 1024), (4092, 1000, 1023)):
        assert L.vivim_token_layernorm_bwd_workspace_bytes(ctypes.byref(_params(rows, C))) == slots * 2 * C * 4
        assert ln.tm_workspace_slots(rows) == slots              # the wrapper sizes the workspace by the header's formula
    assert L.vivim_token_layernorm_bwd_workspace_bytes(None) == 0
    assert L.vivim_token_layernorm_bwd_workspace_bytes(ctypes.byref(_params(C=1025))) == 0
    P = _params(100, 64, _lib.F32, _lib.BF16)
    assert _lib.algorithmic_bytes(FWD, P) == 100 * 64 * (4 + 2) + 8 * 100
    assert _lib.algorithmic_bytes(BWD, P) == 100 * 64 * (4 + 2 + 4) + 8 * 100 + 12 * 64
    P.mean = P.rstd = None                                       # the no-grad forward writes no statistics
    assert _lib.algorithmic_bytes(FWD, P) == 100 * 64 * (4 + 2)


def test_tm_supported_on_the_cpu():
    w = torch.ones(64)
    assert ln.tm_supported(torch.randn(5, 64), w, None) is False                  # a CPU tensor
    meta = torch.device("meta")
    x = torch.empty(3, 7, 64, device=meta)
    # the layout rules, on tensors that have strides but no memory
    assert ln._rows(x) == (21, 64) and ln._rows(x[..., :32]) == (21, 64) and ln._rows(x[:, :5]) is None
    assert ln._rows(x[:, :1]) == (3, 7 * 64) and ln._rows(x[1]) == (7, 64) and ln._rows(x[0, 0]) == (1, 64)
    assert ln._rows(torch.empty(0, 64, device=meta)) is None
    assert ln.tm_pair_ok(torch.float32, torch.bfloat16) and ln.tm_pair_ok(torch.float16, torch.float32)
    assert not ln.tm_pair_ok(torch.float16, torch.bfloat16) and not ln.tm_pair_ok(torch.float64, torch.float64)
    with pytest.raises(ValueError, match="unsupported"):
        ln.layer_norm_tm(torch.randn(5, 64), w, None)


def test_tm_supported_refusals_need_no_gpu(monkeypatch):
    """A bf16 weight and a strided channel axis are refused whatever the device: shown on tensors that claim to be CUDA ones."""
    class Fake:
        def __init__(self, t, cuda=True):
            self.t, self.is_cuda = t, cuda
            self.dtype, self.shape, self.device = t.dtype, t.shape, "cuda:0" if cuda else t.device

        def dim(self): return self.t.dim()
        def stride(self, d): return self.t.stride(d)
        def numel(self): return self.t.numel()
        def is_contiguous(self): return self.t.is_contiguous()

    x, w = Fake(torch.randn(2, 5, 64)), Fake(torch.ones(64))
    assert ln.tm_supported(x, w, None) is True and ln.tm_supported(x, w, Fake(torch.zeros(64))) is True
    assert ln.tm_supported(Fake(torch.randn(2, 5, 64), cuda=False), w, None) is False
    assert ln.tm_supported(x, Fake(torch.ones(64, dtype=torch.bfloat16)), None) is False
    assert ln.tm_supported(x, w, Fake(torch.zeros(64, dtype=torch.bfloat16))) is False
    assert ln.tm_supported(Fake(torch.randn(2, 64, 5).transpose(1, 2)), w, None) is False       # channel stride 5
    assert ln.tm_supported(Fake(torch.randn(2, 5, 128)[..., ::2]), w, None) is False            # channel stride 2
    assert ln.tm_supported(Fake(torch.randn(2, 5, 1025)), Fake(torch.ones(1025)), None) is False
    assert ln.tm_supported(Fake(torch.randn(2, 5, 64).double()), w, None) is False
    assert ln.tm_supported(x, None, None) is False
    monkeypatch.setattr(_lib, "deterministic", lambda: True)                                     # no atomics: still supported
    assert ln.tm_supported(x, w, None) is True


# ---- the swap -------------------------------------------------------------------------------------------------------------------
def _backbone():
    from transformers import SegformerConfig, SegformerForSemanticSegmentation
    cfg = SegformerConfig(num_channels=3, num_encoder_blocks=2, depths=[2, 1], sr_ratios=[2, 1], hidden_sizes=[16, 32],
                          patch_sizes=[7, 3], strides=[4, 2], num_attention_heads=[1, 2], mlp_ratios=[2, 2],
                          decoder_hidden_size=32, num_labels=3)
    torch.manual_seed(41)
    return SegformerForSemanticSegmentation(cfg)


def _blocks(backbone, **kw):
    from vivim_amd.vivim import mamba_block
    return mamba_block(backbone, 3, depths=[0, 0], dims=[16, 32], **kw)


def test_switches_exist_and_default_off():
    from vivim_amd import train_step, vivim
    for fn in (vivim.mamba_block.__init__, vivim.Vivim.__init__, train_step.build_model):
        assert inspect.signature(fn).parameters["fast_backbone_layernorm"].default is False
    # the threshold profiles/r08_layernorm_tm.txt gave: stage 0 of the bench (61440 x 64) is above it, stage 1 (15360 x 128) below
    meta = torch.device("meta")
    assert ln.tm_worthwhile(torch.empty(61440, 64, device=meta)) and not ln.tm_worthwhile(torch.empty(15360, 128, device=meta))


def test_swap_keeps_keys_and_parameter_identity():
    from vivim_amd.vivim import _BackboneLayerNorm, _encoder_parts
    backbone = _backbone()
    before = {n: p for n, p in backbone.named_parameters()}
    stock_keys = list(_blocks(copy.deepcopy(backbone)).state_dict())
    block = _blocks(backbone, fast_backbone_layernorm=True)
    assert list(block.state_dict()) == stock_keys
    after = {n: p for n, p in backbone.named_parameters()}
    assert set(after) == set(before) and all(after[n] is before[n] for n in before)
    enc = block.downsample_layers
    swapped = [(n, m) for n, m in enc.named_modules() if isinstance(m, _BackboneLayerNorm)]
    # per stage: the patch embedding's norm; per block: before, after and, with sr_ratio > 1, the sequence reduction's
    assert len(swapped) == 2 + 2 * 3 + 1 * 2
    assert all(m.low_precision_out == n.startswith("block.") for n, m in swapped)
    assert not any(isinstance(m, _BackboneLayerNorm) for m in enc.layer_norm.modules())     # the stage norms: never called
    assert all(type(m) is torch.nn.LayerNorm for m in _encoder_parts(backbone)[2])
    assert all(m.weight.requires_grad and m.elementwise_affine and m.eps == 1e-5 for _, m in swapped)


def test_swapped_backbone_on_the_cpu_is_the_stock_one_bit_for_bit():
    backbone = _backbone()
    stock = _blocks(copy.deepcopy(backbone)).eval()
    swapped = _blocks(backbone, fast_backbone_layernorm=True).eval()
    x = torch.randn(1, 2, 3, 32, 32, generator=torch.Generator().manual_seed(42))
    # depths = 0: the Mamba stages are empty, the output is the SegFormer stages' alone
    with torch.no_grad():
        a, b = stock(x), swapped(x)
    assert len(a) == len(b) == 2 and all(torch.equal(u, v) for u, v in zip(a, b))
    with torch.autocast("cpu", dtype=torch.bfloat16), torch.no_grad():
        a, b = stock(x), swapped(x)
    assert all(u.dtype == v.dtype and torch.equal(u, v) for u, v in zip(a, b))
