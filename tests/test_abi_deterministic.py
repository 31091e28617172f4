"""CPU: the deterministic backward entry points (vivim_selective_scan_bwd_det and its workspace query) are declared and
exported, size their slot workspace by the formula in include/vivim_hip.h, and refuse a missing or too small workspace and
bad params before anything is launched."""
import ctypes
import os
import re

from conftest import ROOT
from vivim_amd import _lib

NEW = ("vivim_scan_bwd_det_workspace_bytes", "vivim_scan_bwd_det_call_workspace_bytes", "vivim_selective_scan_bwd_det",
       "vivim_causal_conv1d_bwd_det_workspace_bytes", "vivim_causal_conv1d_bwd_det",
       "vivim_dwconv_wgrad_det_workspace_bytes", "vivim_dwconv_wgrad_det")


def _shape(itype, batch, dim, groups, dstate, seqlen, variable=1):
    s = _lib.SsmFwdParams()
    s.batch, s.dim, s.n_groups, s.dstate, s.seqlen, s.itype = batch, dim, groups, dstate, seqlen, itype
    s.is_variable_B = s.is_variable_C = variable
    s.u_d_stride = s.delta_d_stride = s.out_d_stride = s.B_dstate_stride = s.C_dstate_stride = seqlen
    s.u_batch_stride = s.delta_batch_stride = s.out_batch_stride = seqlen * dim
    s.B_group_stride = s.C_group_stride = seqlen * dstate
    s.B_batch_stride = s.C_batch_stride = seqlen * dstate * groups
    return s


def _det_bytes(s):
    return _lib.lib().vivim_scan_bwd_det_workspace_bytes(ctypes.byref(s))


def test_det_symbols_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vivim_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTS
        assert hasattr(L, name)


def test_det_workspace_follows_formula():
    """Generic family: SA = batch slots of dA / dD / dbias, SB slots of dB / dC; every slot written, none shared."""
    prev = (_lib.lib().vivim_set_tuning(0, 0), _lib.lib().vivim_set_tuning(1, 0))
    try:
        b, d, n, l = 2, 64, 16, 1280
        # constant B / C (generic only): SB = batch slots of (dim, dstate)
        assert _det_bytes(_shape(_lib.F32, b, d, 1, n, l, variable=0)) == 4 * (b * d * (n + 2) + 2 * b * d * n)
        # variable B / C with the generic backward pinned: SB = channel pairs per group, slots of (batch, groups, dstate, L)
        _lib.lib().vivim_set_tuning(1, 3)
        s = _shape(_lib.BF16, b, d, 1, 24, l)
        assert _det_bytes(s) >= 4 * (b * d * (24 + 2) + 2 * (d // 2) * b * 24 * l)
        # lanes = tokens / lanes = states shapes: more than two contributors per dA element -> a positive size that covers
        # the generic fallback and grows with the batch
        for tv, dstate in ((1, 64), (2, 16), (4, 16), (5, 16), (0, 64)):
            _lib.lib().vivim_set_tuning(1, tv)
            s4 = _shape(_lib.BF16, 4, 256, 2, dstate, 8192)
            gen = 4 * (4 * 256 * (dstate + 2) + 2 * (128 // 2) * 4 * 2 * dstate * 8192)
            assert _det_bytes(s4) >= gen > 0
            assert _det_bytes(_shape(_lib.BF16, 8, 256, 2, dstate, 8192)) > _det_bytes(s4)
    finally:
        _lib.lib().vivim_set_tuning(0, prev[0])
        _lib.lib().vivim_set_tuning(1, prev[1])
    assert _lib.lib().vivim_scan_bwd_det_workspace_bytes(None) == 0


def _bwd_params():
    p = _lib.SsmBwdParams()
    s = _shape(_lib.F32, 2, 64, 1, 16, 256)
    ctypes.memmove(ctypes.addressof(p.f), ctypes.addressof(s), ctypes.sizeof(s))
    f = p.f
    f.u = f.delta = f.A = f.B = f.C = f.x = 256
    p.dout = p.du = p.ddelta = p.dA = p.dB = p.dC = 256
    return p


def test_det_entry_rejects_before_launch():
    """NULL struct, the existing bad-param cases, and a NULL / too small / misaligned workspace: VIVIM_ERR_INVALID,
    nothing launched (no GPU here: a launch would fail with a different code)."""
    L = _lib.lib()
    assert L.vivim_selective_scan_bwd_det(None, None, 0, None) == 1
    p = _bwd_params()
    need = L.vivim_scan_bwd_det_call_workspace_bytes(ctypes.byref(p))
    assert 0 < need <= L.vivim_scan_bwd_det_workspace_bytes(ctypes.byref(p.f))
    assert L.vivim_selective_scan_bwd_det(ctypes.byref(p), None, need, None) == 1
    assert b"workspace" in L.vivim_last_error()
    assert L.vivim_selective_scan_bwd_det(ctypes.byref(p), 4096, need - 4, None) == 1
    assert L.vivim_selective_scan_bwd_det(ctypes.byref(p), 4100, need, None) == 1      # not 16-byte aligned
    p.dA = None                                                                         # missing gradient output
    assert L.vivim_selective_scan_bwd_det(ctypes.byref(p), 4096, need, None) == 1
    assert b"check failed" in L.vivim_last_error()
    p = _bwd_params()
    p.f.dstate = 300                                                                    # bad dstate
    assert L.vivim_selective_scan_bwd_det(ctypes.byref(p), 4096, 1 << 30, None) == 1
    p = _bwd_params()
    p.f.itype = 7                                                                       # bad dtype
    assert L.vivim_selective_scan_bwd_det(ctypes.byref(p), 4096, 1 << 30, None) == 1


def _call_params(itype, batch, dim, dstate, seqlen):
    """Backward params with aligned (never dereferenced) pointers and the segment workspace the shape asks for."""
    L = _lib.lib()
    p = _lib.SsmBwdParams()
    s = _shape(itype, batch, dim, 1, dstate, seqlen)
    ctypes.memmove(ctypes.addressof(p.f), ctypes.addressof(s), ctypes.sizeof(s))
    p.f.u = p.f.delta = p.f.A = p.f.B = p.f.C = p.f.x = 1 << 20
    p.dout = p.du = p.ddelta = p.dA = p.dB = p.dC = 1 << 20
    p.dout_d_stride = p.du_d_stride = p.ddelta_d_stride = seqlen
    p.dout_batch_stride = p.du_batch_stride = p.ddelta_batch_stride = seqlen * dim
    p.dB_batch_stride = p.dC_batch_stride = seqlen * dstate
    p.dB_group_stride = p.dC_group_stride = seqlen * dstate
    p.dB_dstate_stride = p.dC_dstate_stride = seqlen
    ws = L.vivim_scan_bwd_workspace_bytes(ctypes.byref(p.f))
    p.workspace, p.workspace_bytes = (1 << 24) if ws else None, ws
    unit = batch * dim * (2 * dstate + 1) * 4                       # segment records per (batch, channel, segment)
    return p, max(1, ws // unit)


def test_det_call_workspace_exact_per_family():
    """The call-level size is the header formula of the family the call runs: lanes = tokens (4 waves) and lanes = states
    first generation with more than two workgroups per group (dB / dC slotted) and with two (dB / dC not slotted)."""
    L = _lib.lib()
    prev = (L.vivim_set_tuning(0, 0), L.vivim_set_tuning(1, 0))
    try:
        b, n, l = 2, 16, 4096
        L.vivim_set_tuning(0, 1)
        L.vivim_set_tuning(1, 2)                                    # lanes = tokens, 4 waves
        d = 256
        p, S = _call_params(_lib.BF16, b, d, n, l)
        sb = ((d + 1) // 2 + 3) // 4
        assert L.vivim_scan_bwd_det_call_workspace_bytes(ctypes.byref(p)) == 4 * (b * S * d * (n + 2) + 2 * sb * b * n * l)
        L.vivim_set_tuning(0, 6)
        L.vivim_set_tuning(1, 4)                                    # lanes = states, first generation: W = 4, 64 channels per wg
        for d, sb in ((256, 4), (128, 0)):
            p, S = _call_params(_lib.BF16, b, d, n, l)
            assert L.vivim_scan_bwd_det_call_workspace_bytes(ctypes.byref(p)) == 4 * (b * S * d * (n + 2) + 2 * sb * b * n * l)
            assert L.vivim_scan_bwd_det_call_workspace_bytes(ctypes.byref(p)) <= _det_bytes(p.f)
    finally:
        L.vivim_set_tuning(0, prev[0])
        L.vivim_set_tuning(1, prev[1])


def _conv_bwd_params():
    """Conv1d backward params that pass every check (never dereferenced pointers) and their det workspace size."""
    f = _lib.ConvFwdParams()
    f.batch, f.dim, f.seqlen, f.width, f.itype, f.wtype = 2, 64, 4096, 4, _lib.BF16, _lib.F32
    f.x_batch_stride, f.x_c_stride, f.x_l_stride = 64 * 4096, 4096, 1
    f.x = f.weight = 1 << 20
    need = _lib.lib().vivim_causal_conv1d_bwd_det_workspace_bytes(ctypes.byref(f))
    p = _lib.ConvBwdParams()
    ctypes.memmove(ctypes.addressof(p.f), ctypes.addressof(f), ctypes.sizeof(f))
    p.dout = p.dx = p.dweight = 1 << 20
    p.dout_l_stride = p.dx_l_stride = 1
    return p, need


def _dw_wgrad_params():
    """Depthwise weight-gradient params that pass every check and their det workspace size."""
    w = _lib.DwConvWgradParams()
    w.batch, w.depth, w.height, w.width, w.channels, w.kd, w.itype = 2, 3, 16, 16, 64, 3, _lib.BF16
    w.x = w.dy = w.dwt = 1 << 20
    w.x_token_stride = w.dy_token_stride = 64
    w.x_batch_stride = w.dy_batch_stride = 64 * 768
    return w, _lib.lib().vivim_dwconv_wgrad_det_workspace_bytes(ctypes.byref(w))


def test_conv_and_dwconv_det_reject_before_launch():
    L = _lib.lib()
    p, need = _conv_bwd_params()
    assert need == 4 * 2 * (4096 // 2048) * 64 * 5                # batch * tiles of 256 x 8 tokens, dim * (width + 1)
    assert L.vivim_causal_conv1d_bwd_det(ctypes.byref(p), None, need, None) == 1
    assert L.vivim_causal_conv1d_bwd_det(ctypes.byref(p), 4096, need - 4, None) == 1
    p.f.width = 5
    assert L.vivim_causal_conv1d_bwd_det(ctypes.byref(p), 4096, need, None) == 1
    w, dneed = _dw_wgrad_params()
    assert dneed > 0 and dneed % (4 * 28 * 64 * 2) == 0           # whole (batch, block) slots of 28 x channels floats
    assert L.vivim_dwconv_wgrad_det(ctypes.byref(w), None, dneed, None) == 1
    assert L.vivim_dwconv_wgrad_det(ctypes.byref(w), 4096, dneed - 4, None) == 1
    w.kd = 2
    assert L.vivim_dwconv_wgrad_det(ctypes.byref(w), 4096, 1 << 30, None) == 1
