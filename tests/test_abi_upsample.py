"""CPU: the bilinear-upsampling entry points (include/vivim_hip.h: vivim_upsample_params) are declared, exported and present,
the ctypes mirror has the library's layout, every bad argument is refused on the host before any launch, and on CPU tensors
vivim_amd.bilinear_upsample IS F.interpolate, bit for bit, forward and gradient."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from vivim_amd import _lib

NAMES = ("vivim_upsample_bilinear2d_fwd", "vivim_upsample_bilinear2d_bwd")
OK, INVALID, UNSUPPORTED = 0, 1, 2
PTR = 1 << 20                                    # a non-null, 16-byte aligned address: no check may dereference it


def test_symbols_declared_exported_and_present():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vivim_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vivim_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTS and hasattr(L, n), n
        assert getattr(L, n).argtypes == [ctypes.POINTER(_lib.UpsampleParams), ctypes.c_void_p]
    assert "vivim_upsample_params" in text


def test_struct_layout_and_abi_version():
    L = _lib.lib()
    assert L.vivim_sizeof(14) == ctypes.sizeof(_lib.UpsampleParams) > 0
    assert L.vivim_sizeof(99) == 0
    assert L.vivim_abi_version() == 8
    names = [f[0] for f in _lib.UpsampleParams._fields_]
    assert names == ["batch", "channels", "in_h", "in_w", "out_h", "out_w", "itype", "layout", "x_batch_stride",
                     "y_batch_stride", "x", "y", "dy", "dx"]


def _params(N=2, C=8, H=5, W=7, OH=20, OW=28, itype=_lib.F32, layout=0):
    P = _lib.UpsampleParams()
    P.batch, P.channels, P.in_h, P.in_w, P.out_h, P.out_w, P.itype, P.layout = N, C, H, W, OH, OW, itype, layout
    P.x_batch_stride, P.y_batch_stride = C * H * W, C * OH * OW
    P.x = P.y = P.dy = P.dx = PTR
    return P


def _refused(P, code, message=None, names=NAMES):
    """`code` and nothing launched: the pointers are not memory, so a kernel that started would not return an error code."""
    L = _lib.lib()
    for n in names:
        assert getattr(L, n)(ctypes.byref(P), None) == code, (n, L.vivim_last_error())
        assert L.vivim_last_error() != b""
        if message is not None:
            assert message in L.vivim_last_error(), L.vivim_last_error()


def test_null_struct_and_null_pointers():
    L = _lib.lib()
    for n in NAMES:
        assert getattr(L, n)(None, None) == INVALID and b"check failed" in L.vivim_last_error()
    for layout in (0, 1):
        # each call refuses the absence of the pointers IT needs, whatever the other two are
        for field, name in (("x", NAMES[0]), ("y", NAMES[0]), ("dy", NAMES[1]), ("dx", NAMES[1])):
            P = _params(layout=layout)
            setattr(P, field, None)
            _refused(P, INVALID, b"check failed", names=(name,))


def test_misaligned_pointers():
    for itype, offs in ((_lib.F32, (1, 2)), (_lib.F16, (1,)), (_lib.BF16, (1,))):
        for off in offs:
            for field, name in (("x", NAMES[0]), ("y", NAMES[0]), ("dy", NAMES[1]), ("dx", NAMES[1])):
                P = _params(itype=itype, layout=1)
                setattr(P, field, PTR + off)
                _refused(P, INVALID, b"check failed", names=(name,))


def test_bad_sizes_types_and_layouts():
    for field, v in (("batch", 0), ("batch", -1), ("channels", 0), ("in_h", 0), ("in_w", -2), ("out_h", 0), ("out_w", -1),
                     ("itype", 3), ("itype", -1), ("layout", 2), ("layout", -1)):
        P = _params()
        setattr(P, field, v)
        _refused(P, INVALID, b"check failed")


def test_downsampling_is_unsupported_with_a_message():
    for kw in (dict(H=21), dict(W=29), dict(H=40, W=56), dict(H=21, layout=1)):
        _refused(_params(**kw), UNSUPPORTED, b"upsampling only")


def test_sizes_past_31_bits_are_refused():
    for kw in (dict(C=1 << 16, OH=1 << 8, OW=1 << 8),                    # one output image of 2^32 elements
               dict(C=1 << 16, OH=1 << 8, OW=1 << 8, layout=1),
               dict(C=1, H=1 << 15, W=1, OH=1 << 15, OW=1),              # (2 in_h + 3) * out_h
               dict(C=1, H=1, W=1 << 15, OH=1, OW=1 << 15, layout=1),    # (2 in_w + 3) * out_w
               dict(N=1 << 20, C=1 << 11),                               # N * C planes
               dict(N=1 << 17, C=1, H=1, W=1, OH=1 << 14, OW=1)):        # N * out_h rows
        _refused(_params(**kw), INVALID, b"check failed")
    # 2^20 planes of 64 x 32 forward tiles: 2^31 workgroups (the backward's 2^20 are fine, so it is not called here)
    _refused(_params(N=1 << 12, C=1 << 8, H=1, W=1, OH=1 << 10, OW=1 << 11), INVALID, b"check failed", names=NAMES[:1])


def test_algorithmic_bytes_has_a_branch_for_the_new_names():
    P = _params(N=2, C=3, H=4, W=5, OH=8, OW=15, itype=_lib.BF16)
    for n in NAMES:
        assert _lib.algorithmic_bytes(n, P) == 2 * 3 * (20 + 120) * 2
    P.itype = _lib.F32
    assert _lib.algorithmic_bytes(NAMES[1], P) == 2 * 3 * (20 + 120) * 4


def test_exported_from_the_package():
    import vivim_amd
    from vivim_amd import upsample
    assert vivim_amd.bilinear_upsample is upsample.bilinear_upsample
    with pytest.raises(AttributeError):
        vivim_amd.no_such_name


def test_supported_is_false_for_cpu_tensors():
    from vivim_amd import upsample
    for x in (torch.randn(2, 3, 4, 5), torch.randn(2, 8, 4, 5).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)):
        assert upsample.supported(x, (8, 10)) is False


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
@pytest.mark.parametrize("channels_last", (False, True))
@pytest.mark.parametrize("size", ((9, 11), (4, 5), (3, 8)))           # up, equal, down on one axis
def test_cpu_tensors_are_f_interpolate_bit_for_bit(size, channels_last, dtype):
    from vivim_amd import bilinear_upsample
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 6, 4, 5, generator=g).to(dtype)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    go = torch.randn(2, 6, *size, generator=g).to(dtype)
    a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya = bilinear_upsample(a, size)
    yb = F.interpolate(b, size=size, mode="bilinear", align_corners=False)
    assert ya.dtype == yb.dtype and ya.stride() == yb.stride() and torch.equal(ya, yb)
    ya.backward(go)
    yb.backward(go)
    assert torch.equal(a.grad, b.grad)


def test_the_switch_exists_and_is_off_by_default():
    from vivim_amd import train_step, vivim
    assert inspect.signature(vivim.Vivim.__init__).parameters["fused_upsample"].default is False
    assert inspect.signature(train_step.build_model).parameters["fused_upsample"].default is False
