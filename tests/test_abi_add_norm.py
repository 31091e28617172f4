"""CPU: the residual-add LayerNorm entry points (include/vivim_hip.h: vivim_add_layernorm_params) are declared, exported and
present, the ctypes mirror has the library's layout, and every bad argument is refused on the host before any launch."""
import ctypes
import os
import re

from conftest import ROOT
from vivim_amd import _lib

NAMES = ("vivim_add_layernorm_cm_fwd", "vivim_add_layernorm_cm_bwd", "vivim_add_layernorm_bwd_workspace_bytes")
OK, INVALID, UNSUPPORTED = 0, 1, 2
PTR = 1 << 20                                    # a non-null, 16-byte aligned address: no check may dereference it


def test_symbols_declared_exported_and_present():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vivim_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vivim_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTS and hasattr(L, n), n
    assert "vivim_add_layernorm_params" in text


def test_struct_layout_and_abi_version():
    L = _lib.lib()
    assert L.vivim_sizeof(11) == ctypes.sizeof(_lib.AddLayerNormParams) > 0
    assert L.vivim_abi_version() == 8


def _params(itype=_lib.F32, btype=None, otype=None, B=2, L=64, C=32, norm=True, bwd=False):
    P = _lib.AddLayerNormParams()
    P.batch, P.seqlen, P.channels = B, L, C
    P.itype, P.btype, P.otype, P.eps = itype, itype if btype is None else btype, itype if otype is None else otype, 1e-5
    P.x_batch_stride = P.x_new_batch_stride = P.dres_batch_stride = P.dx_batch_stride = C * L
    P.x_c_stride = P.x_new_c_stride = P.dres_c_stride = P.dx_c_stride = L
    P.branch_batch_stride = P.y_batch_stride = P.dbranch_batch_stride = L * C
    P.branch_token_stride = P.y_token_stride = P.dbranch_token_stride = C
    P.x = P.branch = P.x_new = PTR
    if norm:
        P.weight = P.bias = P.y = P.mean = P.rstd = PTR
    if bwd:
        P.dres = P.dbranch = PTR
        if norm:
            P.dy = P.dx = PTR
    return P


def _rc(fn, P):
    return getattr(_lib.lib(), fn)(ctypes.byref(P), None)


def _refused(fn, P, code, message=None):
    """`code` and nothing launched: the pointers are not memory, so a kernel that started would not return an error code."""
    assert _rc(fn, P) == code, _lib.lib().vivim_last_error()
    if message is not None:
        assert message in _lib.lib().vivim_last_error(), _lib.lib().vivim_last_error()


FWD, BWD = "vivim_add_layernorm_cm_fwd", "vivim_add_layernorm_cm_bwd"


def test_null_struct_and_null_pointers():
    L = _lib.lib()
    assert L.vivim_add_layernorm_cm_fwd(None, None) == INVALID and b"check failed" in L.vivim_last_error()
    assert L.vivim_add_layernorm_cm_bwd(None, None) == INVALID
    assert L.vivim_add_layernorm_bwd_workspace_bytes(None) == 0
    for field in ("x", "branch", "x_new", "y", "mean", "rstd"):
        P = _params()
        setattr(P, field, None)
        _refused(FWD, P, INVALID, b"check failed")
    for field in ("x", "branch", "x_new"):                          # add-only forward
        P = _params(norm=False)
        setattr(P, field, None)
        _refused(FWD, P, INVALID)
    for field in ("x_new", "mean", "rstd", "dx"):
        P = _params(bwd=True)
        setattr(P, field, None)
        _refused(BWD, P, INVALID)
    P = _params(bwd=True)                                            # dy or dres may be absent, not both
    P.dy = P.dres = None
    _refused(BWD, P, INVALID)
    for field in ("dres", "dbranch"):                                # add-only backward needs both
        P = _params(norm=False, bwd=True)
        setattr(P, field, None)
        _refused(BWD, P, INVALID)


def test_misaligned_pointers_strides_and_seqlen():
    for field in ("x", "x_new"):
        P = _params()
        setattr(P, field, PTR + 4)
        _refused(FWD, P, INVALID)
    for field in ("x_batch_stride", "x_c_stride", "x_new_batch_stride", "x_new_c_stride"):
        P = _params()
        setattr(P, field, getattr(P, field) + 2)                     # f32: vectors of 4 tokens
        _refused(FWD, P, INVALID)
    P = _params(L=66)
    _refused(FWD, P, INVALID)
    P = _params(itype=_lib.BF16, L=68)                               # 16-bit: vectors of 8 tokens
    _refused(FWD, P, INVALID)
    P = _params(itype=_lib.BF16)
    P.x_c_stride += 4
    _refused(FWD, P, INVALID)
    for field in ("x_new", "dres", "dx"):
        P = _params(bwd=True)
        setattr(P, field, PTR + 8)
        _refused(BWD, P, INVALID)
    for field in ("x_new_batch_stride", "x_new_c_stride", "dres_batch_stride", "dres_c_stride", "dx_batch_stride", "dx_c_stride"):
        P = _params(bwd=True)
        setattr(P, field, getattr(P, field) + 1)
        _refused(BWD, P, INVALID)
    P = _params(norm=False, bwd=True)
    P.dres = PTR + 4
    _refused(BWD, P, INVALID)
    P = _params(bwd=True, L=62)
    _refused(BWD, P, INVALID)
    for bad in (dict(B=0), dict(L=0), dict(C=0), dict(B=70000)):
        _refused(FWD, _params(**bad), INVALID)
    P = _params()
    P.itype = 7
    _refused(FWD, P, INVALID)


def test_unsupported_channels_and_dtype_pairs_carry_a_message():
    for fn, bwd in ((FWD, False), (BWD, True)):
        _refused(fn, _params(C=1024, bwd=bwd), UNSUPPORTED, b"512 channels")
        _refused(fn, _params(C=1024, bwd=bwd, norm=False), UNSUPPORTED, b"512 channels")
        _refused(fn, _params(itype=_lib.BF16, btype=_lib.F32, bwd=bwd), UNSUPPORTED, b"branch type")      # x 16-bit, branch f32
        _refused(fn, _params(itype=_lib.BF16, btype=_lib.F16, bwd=bwd), UNSUPPORTED, b"branch type")
        _refused(fn, _params(itype=_lib.F16, btype=_lib.BF16, bwd=bwd, norm=False), UNSUPPORTED, b"branch type")
        _refused(fn, _params(itype=_lib.F32, otype=_lib.BF16, bwd=bwd), UNSUPPORTED, b"output type")       # y is f32 or x's type
        _refused(fn, _params(itype=_lib.BF16, otype=_lib.F16, bwd=bwd), UNSUPPORTED, b"output type")


def test_dweight_dbias_need_the_workspace():
    for field in ("dweight", "dbias"):
        P = _params(bwd=True)
        setattr(P, field, PTR)
        _refused(BWD, P, INVALID, b"workspace")


def test_workspace_bytes_follow_the_layernorm_tile_choice(monkeypatch):
    """A row of 2 C floats per tile, with the tile length (and its VIVIM_LN_TT override) of vivim_layernorm_bwd_workspace_bytes."""
    L = _lib.lib()
    for tile in (None, "8", "16", "32"):
        if tile is None:
            monkeypatch.delenv("VIVIM_LN_TT", raising=False)
        else:
            monkeypatch.setenv("VIVIM_LN_TT", tile)
        for itype, B, T, C in ((_lib.F32, 2, 1000, 64), (_lib.BF16, 3, 320, 512), (_lib.F32, 3, 20480, 64), (_lib.F16, 1, 40, 96)):
            P = _params(itype=itype, B=B, L=T, C=C)
            Q = _lib.LayerNormParams()
            Q.batch, Q.seqlen, Q.channels, Q.itype, Q.otype = B, T, C, itype, itype
            want = L.vivim_layernorm_bwd_workspace_bytes(ctypes.byref(Q))
            assert want > 0 and L.vivim_add_layernorm_bwd_workspace_bytes(ctypes.byref(P)) == want


def test_algorithmic_bytes_has_a_branch_for_the_new_names():
    P = _params(itype=_lib.F32, btype=_lib.BF16, B=2, L=64, C=32)
    n = 2 * 64 * 32
    assert _lib.algorithmic_bytes(FWD, P) == n * (4 + 4 + 2 + 4) + 8 * 2 * 64 + 8 * 32
    A = _params(itype=_lib.F32, btype=_lib.BF16, B=2, L=64, C=32, norm=False, bwd=True)
    assert _lib.algorithmic_bytes(FWD, A) == n * (4 + 4 + 2) and _lib.algorithmic_bytes(BWD, A) == n * (4 + 2)
    Pb = _params(itype=_lib.F32, btype=_lib.BF16, B=2, L=64, C=32, bwd=True)
    assert _lib.algorithmic_bytes(BWD, Pb) == n * (4 + 4 + 4 + 4 + 2) + 8 * 2 * 64 + 12 * 32
