"""CPU: vivim_selective_scan_fwd_lean (include/vivim_hip.h) is declared, exported and present, the ABI version and the params
layout did not move, and every bad argument is refused on the host before any launch."""
import ctypes
import os
import re

from conftest import ROOT
from vivim_amd import _lib

LEAN, FULL = "vivim_selective_scan_fwd_lean", "vivim_selective_scan_fwd"
OK, INVALID, UNSUPPORTED = 0, 1, 2
PTR = 1 << 20                                    # a non-null, 16-byte aligned address: no check may dereference it
REQUIRED = ("u", "delta", "A", "B", "C")


def test_symbol_declared_exported_and_present():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vivim_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vivim_[a-z0-9_]+)\s*\(", text))
    assert LEAN in declared and LEAN in _lib.EXPORTS and hasattr(_lib.lib(), LEAN)
    assert re.search(r"int\s+vivim_selective_scan_fwd_lean\s*\(\s*const\s+vivim_ssm_fwd_params\s*\*\s*\w+\s*,\s*void\s*\*\s*last_state\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", text)


def test_abi_version_and_params_layout_did_not_move():
    L = _lib.lib()
    assert L.vivim_abi_version() == 8
    assert L.vivim_sizeof(0) == ctypes.sizeof(_lib.SsmFwdParams) > 0
    header = open(os.path.join(ROOT, "include", "vivim_hip.h")).read()
    assert re.search(r"#define VIVIM_ABI_VERSION 8\b", header)


def _params(z=True, itype=_lib.F32, B=2, D=64, L=256, N=16, G=1, var=(1, 1)):
    """What fwd_lean passes for a (B, D, L) problem: x NULL; with z out_z alone, without z out."""
    P = _lib.SsmFwdParams()
    P.batch, P.dim, P.seqlen, P.dstate, P.n_groups, P.itype = B, D, L, N, G, itype
    P.is_variable_B, P.is_variable_C, P.delta_softplus = var[0], var[1], 1
    P.u_batch_stride = P.delta_batch_stride = P.z_batch_stride = P.out_batch_stride = P.out_z_batch_stride = D * L
    P.u_d_stride = P.delta_d_stride = P.z_d_stride = P.out_d_stride = P.out_z_d_stride = L
    P.A_d_stride, P.A_dstate_stride = N, 1
    P.B_batch_stride = P.C_batch_stride = G * N * L
    P.B_group_stride = P.C_group_stride = N * L
    P.B_dstate_stride = P.C_dstate_stride = L
    P.u = P.delta = P.A = P.B = P.C = P.D = P.delta_bias = PTR
    if z:
        P.z = P.out_z = PTR
    else:
        P.out = PTR
    return P


def _refused(P, code, message=None, fn=LEAN, last_state=None):
    """`code` and nothing launched: the pointers are not memory, so a kernel that started would not return an error code."""
    L = _lib.lib()
    rc = L.vivim_selective_scan_fwd_lean(ctypes.byref(P), last_state, None) if fn == LEAN else L.vivim_selective_scan_fwd(ctypes.byref(P), None)
    assert rc == code, (rc, L.vivim_last_error())
    assert rc != OK and L.vivim_last_error(), "a refusal sets vivim_last_error()"
    if message is not None:
        assert message in L.vivim_last_error(), L.vivim_last_error()


def test_null_struct_is_refused():
    L = _lib.lib()
    assert L.vivim_selective_scan_fwd_lean(None, None, None) == INVALID and b"check failed" in L.vivim_last_error()
    assert L.vivim_selective_scan_fwd_lean(None, PTR, None) == INVALID


def test_every_required_pointer_is_checked():
    for z in (True, False):
        for field in REQUIRED:
            P = _params(z=z)
            setattr(P, field, None)
            _refused(P, INVALID, b"check failed")


def test_x_must_be_null():
    for z in (True, False):
        P = _params(z=z)
        P.x = PTR
        _refused(P, INVALID, b"x must be NULL")
        _refused(P, INVALID, b"x must be NULL", last_state=PTR)


def test_outputs_with_and_without_z():
    P = _params(z=True)
    P.out = PTR                                   # with z only out_z is written
    _refused(P, INVALID, b"out must be NULL")
    P = _params(z=True)
    P.out_z = None
    _refused(P, INVALID)
    P = _params(z=False)
    P.out = None
    _refused(P, INVALID)
    P = _params(z=False)                          # out_z without z is not a substitute for out
    P.out, P.out_z = None, PTR
    _refused(P, INVALID)


def test_mixed_constant_and_variable_bc_is_unsupported():
    for var in ((1, 0), (0, 1)):
        for z in (True, False):
            _refused(_params(z=z, var=var), UNSUPPORTED, b"mixed constant/variable")


def test_bad_itype_sizes_and_dstate():
    P = _params()
    P.itype = 7
    _refused(P, INVALID)
    _refused(_params(N=257), INVALID)
    _refused(_params(N=512, z=False), INVALID)
    for bad in (dict(B=0), dict(D=0), dict(L=0), dict(N=0), dict(G=0), dict(D=64, G=3)):
        _refused(_params(**bad), INVALID)
    P = _params(var=(0, 0), G=2, D=64)            # constant B / C have one group
    _refused(P, INVALID)


def test_the_full_entry_point_keeps_its_checks():
    P = _params(z=True)
    P.out = PTR                                   # everything the full call wants but x
    _refused(P, INVALID, b"check failed", fn=FULL)
    P = _params(z=False)
    _refused(P, INVALID, b"check failed", fn=FULL)
    P = _params(z=True)                           # x given, out missing
    P.x = PTR
    _refused(P, INVALID, b"check failed", fn=FULL)


def test_algorithmic_bytes_of_the_lean_forward():
    """u, delta, z, out_z (or u, delta, out) + B, C + A, D, delta_bias: one activation tensor fewer than the full call with z."""
    P = _params(z=True, itype=_lib.BF16, B=3, D=384, L=2048, N=16, G=3)
    act, bc, small = 3 * 384 * 2048 * 2, 3 * 3 * 16 * 2048 * 2, 4 * (384 * 16 + 2 * 384)
    assert _lib.algorithmic_bytes(LEAN, P) == 4 * act + 2 * bc + small
    assert _lib.algorithmic_bytes(FULL, P) == 5 * act + 2 * bc + small
    Q = _params(z=False, itype=_lib.BF16, B=3, D=384, L=2048, N=16, G=3)
    assert _lib.algorithmic_bytes(LEAN, Q) == _lib.algorithmic_bytes(FULL, Q) == 3 * act + 2 * bc + small
