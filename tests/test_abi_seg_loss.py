"""CPU: the fused segmentation-loss entry points (include/vivim_hip.h: vivim_seg_loss_params) are declared, exported and present,
the ctypes mirror has the library's layout, every bad argument is refused on the host before any launch, and the Python wrapper
hands CPU tensors to the eager loss unchanged."""
import ctypes
import os
import re

import torch

from conftest import ROOT
from vivim_amd import _lib

NAMES = ("vivim_seg_loss_fwd", "vivim_seg_loss_bwd", "vivim_seg_loss_workspace_bytes")
OK, INVALID, UNSUPPORTED = 0, 1, 2
PTR = 1 << 20                                    # a non-null, 16-byte aligned address: no check may dereference it
FWD, BWD = "vivim_seg_loss_fwd", "vivim_seg_loss_bwd"


def test_symbols_declared_exported_and_present():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vivim_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vivim_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTS and hasattr(L, n), n
    assert "vivim_seg_loss_params" in text


def test_struct_layout_and_abi_version():
    L = _lib.lib()
    assert L.vivim_sizeof(12) == ctypes.sizeof(_lib.SegLossParams) > 0
    assert L.vivim_sizeof(99) == 0
    assert L.vivim_abi_version() == 8


def _sizes(N=2, C=3, HW=35, itype=_lib.F32, ttype=0):
    P = _lib.SegLossParams()
    P.batch, P.classes, P.pixels, P.itype, P.ttype = N, C, HW, itype, ttype
    P.gamma, P.focal_weight, P.tversky_weight = 2.0, 0.4, 0.6
    P.tversky_alpha, P.tversky_beta, P.smooth, P.eps = 0.3, 0.7, 1e-6, 1e-6
    P.logits_batch_stride = P.dlogits_batch_stride = C * HW
    P.logits_c_stride = P.dlogits_c_stride = P.target_batch_stride = HW
    return P


def _params(bwd=False, **kw):
    P = _sizes(**kw)
    P.logits = P.target = P.alpha = PTR
    if bwd:
        P.coef = P.grad_out = P.dlogits = PTR
    else:
        P.loss = P.coef = P.workspace = PTR
        P.workspace_bytes = _lib.lib().vivim_seg_loss_workspace_bytes(ctypes.byref(P))
    return P


def _refused(fn, P, code, message=None):
    """`code` and nothing launched: the pointers are not memory, so a kernel that started would not return an error code."""
    L = _lib.lib()
    assert getattr(L, fn)(ctypes.byref(P), None) == code, L.vivim_last_error()
    assert L.vivim_last_error() != b""
    if message is not None:
        assert message in L.vivim_last_error(), L.vivim_last_error()


def test_null_struct_and_null_pointers():
    L = _lib.lib()
    assert L.vivim_seg_loss_fwd(None, None) == INVALID and b"check failed" in L.vivim_last_error()
    assert L.vivim_seg_loss_bwd(None, None) == INVALID and b"check failed" in L.vivim_last_error()
    assert L.vivim_seg_loss_workspace_bytes(None) == 0
    for field in ("logits", "target", "alpha", "loss", "workspace"):
        P = _params()
        setattr(P, field, None)
        _refused(FWD, P, INVALID)
    for field in ("logits", "target", "alpha", "coef", "grad_out", "dlogits"):
        P = _params(bwd=True)
        setattr(P, field, None)
        _refused(BWD, P, INVALID, b"check failed")


def test_misaligned_pointers():
    for field, off in (("logits", 2), ("target", 4), ("alpha", 2), ("loss", 2), ("coef", 1), ("workspace", 2)):
        P = _params()                                                # f32 logits, int64 target
        setattr(P, field, PTR + off)
        _refused(FWD, P, INVALID)
    P = _params(itype=_lib.BF16)
    P.logits = PTR + 1
    _refused(FWD, P, INVALID)
    for field, off in (("logits", 2), ("target", 4), ("alpha", 2), ("coef", 2), ("grad_out", 2), ("dlogits", 2)):
        P = _params(bwd=True)
        setattr(P, field, PTR + off)
        _refused(BWD, P, INVALID)
    P = _params(bwd=True, itype=_lib.F16)
    P.dlogits = PTR + 1
    _refused(BWD, P, INVALID)


def test_bad_sizes_and_types():
    for fn, bwd in ((FWD, False), (BWD, True)):
        for bad in (dict(HW=0), dict(HW=-3), dict(N=0), dict(N=-1)):
            P = _params(bwd=bwd)                                     # pointers and workspace of a good shape, then the bad size
            for k, v in bad.items():
                setattr(P, {"HW": "pixels", "N": "batch"}[k], v)
            _refused(fn, P, INVALID, b"check failed")
        for field, v in (("itype", 3), ("itype", -1), ("ttype", 2), ("ttype", -1)):
            P = _params(bwd=bwd)
            setattr(P, field, v)
            _refused(fn, P, INVALID, b"check failed")


def test_workspace_one_byte_short():
    P = _params()
    P.workspace_bytes -= 1
    _refused(FWD, P, INVALID, b"vivim_seg_loss_workspace_bytes")
    P.workspace_bytes = 0
    _refused(FWD, P, INVALID, b"workspace")


def test_unsupported_classes_and_gamma_carry_a_message():
    for fn, bwd in ((FWD, False), (BWD, True)):
        for C in (1, 9, 64):
            _refused(fn, _params(bwd=bwd, C=C), UNSUPPORTED, b"2 to 8 classes")
        for gamma in (3.0, 1.0, 0.0):
            P = _params(bwd=bwd)
            P.gamma = gamma
            _refused(fn, P, UNSUPPORTED, b"gamma = 2")


def test_workspace_query_depends_on_sizes_only():
    L = _lib.lib()
    for kw in (dict(), dict(N=3, C=8, HW=5000, itype=_lib.BF16, ttype=1), dict(N=40, C=3, HW=512 * 512, itype=_lib.F16)):
        bare, full = _sizes(**kw), _params(**kw)
        a, b = L.vivim_seg_loss_workspace_bytes(ctypes.byref(bare)), L.vivim_seg_loss_workspace_bytes(ctypes.byref(full))
        assert a == b > 0 and a % (4 * kw.get("N", 2) * (3 * kw.get("C", 3) + 1)) == 0
    # more pixels never need fewer slots, and the slot count per image is capped (the finalise kernel stays tiny)
    sizes = [L.vivim_seg_loss_workspace_bytes(ctypes.byref(_sizes(N=1, C=3, HW=hw))) for hw in (1, 1024, 1025, 4096, 1 << 20, 1 << 28)]
    assert sizes == sorted(sizes) and sizes[0] == 4 * 10 and sizes[-1] == sizes[-2]


def test_algorithmic_bytes_has_a_branch_for_the_new_names():
    P = _sizes(N=2, C=3, HW=100, itype=_lib.BF16, ttype=1)
    assert _lib.algorithmic_bytes(FWD, P) == 200 * (3 * 2 + 1) + 8 * 6
    assert _lib.algorithmic_bytes(BWD, P) == 200 * (2 * 3 * 2 + 1) + 8 * 6


def _cpu_case(dtype=torch.float32):
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(2, 3, 5, 7, generator=g).to(dtype)
    targets = torch.randint(0, 3, (2, 5, 7), generator=g)
    return logits, targets


def test_supported_is_false_for_cpu_tensors():
    from vivim_amd import seg_loss
    logits, targets = _cpu_case()
    assert seg_loss.supported(logits, targets, 3, 2.0) is False
    assert seg_loss.supported(logits, targets.to(torch.uint8), 3, 2.0) is False


def test_cpu_tensors_take_the_eager_loss_exactly():
    from vivim_amd import seg_loss, train_step
    for dtype in (torch.float32, torch.bfloat16):
        logits, targets = _cpu_case(dtype)
        a = logits.clone().requires_grad_(True)
        b = logits.clone().requires_grad_(True)
        la = seg_loss.recall_focused_loss_fused(a, targets, 3)
        lb = train_step.recall_focused_loss(b, targets, 3)
        assert torch.equal(la, lb)
        la.backward()
        lb.backward()
        assert torch.equal(a.grad, b.grad)
    logits, targets = _cpu_case()
    alpha = (0.2, 0.3, 0.5)
    assert torch.equal(seg_loss.recall_focused_loss_fused(logits, targets, 3, 2.0, alpha),
                       train_step.recall_focused_loss(logits, targets, 3, 2.0, alpha=alpha))
    assert torch.equal(seg_loss.recall_focused_loss_fused(logits, targets, 3, gamma=3.0),
                       train_step.recall_focused_loss(logits, targets, 3, gamma=3.0))


def test_train_step_has_the_switch_and_it_is_off_by_default():
    import inspect
    from vivim_amd import train_step
    assert inspect.signature(train_step.train_step).parameters["fused_loss"].default is False
