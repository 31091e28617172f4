"""CPU: the structure loss below the GPU.  The extension header include/vivim_hip_ext.h parses into its row of _lib.EXTENSIONS (what
the registry as a whole holds: test_abi_extensions.py); the struct's layout is the C compiler's; every host-side refusal of the three
entry points, with its message, through _lib.call and directly; the eager functions against the reference's formula written out per
pixel in fp64 and against the fixtures the reference's own functions produced (tests/golden/structloss_*.npz); the kernels'
arithmetic restated in torch fp32 (structure_loss_cases.restate32) held to the GPU test's bounds on the GPU test's inputs; and the
CPU side of `supported` and of the `criterion` keyword."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import structure_loss_cases as sc
from abi_cases import PTR, layout_matches_c, refused as _refused
from conftest import GOLDEN, ROOT
from vivim_amd import _lib
from vivim_amd import structure_loss as sl

HEADER = os.path.join(ROOT, "include", "vivim_hip_ext.h")
NAMES = ("vivim_structure_loss_workspace_bytes", "vivim_structure_loss_fwd", "vivim_structure_loss_bwd")
P = _lib.StructureLossParams


# ---- the header and the tables

def test_the_extension_header_parses_into_its_own_tables():
    struct_names, entry_points = _lib.EXTENSIONS["vivim_hip_ext.h"]
    consts, classes, entries = _lib.parse_header(open(HEADER).read(), struct_names)
    assert consts == {} and list(classes) == ["StructureLossParams"] and tuple(entries) == NAMES
    assert tuple(entry_points) == NAMES and struct_names == {"vivim_structure_loss_params": "StructureLossParams"}
    size_t, c_int, ptr = ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(P)
    assert entry_points == {NAMES[0]: _lib.Entry(None, (ptr,), False, size_t), NAMES[1]: _lib.Entry(None, (ptr,), True, c_int),
                            NAMES[2]: _lib.Entry(None, (ptr,), True, c_int)}
    assert [n for n, _ in P._fields_] == [
        "struct_bytes", "batch", "classes", "height", "width", "itype", "ttype", "first_class", "eps", "_pad0", "logits_batch_stride",
        "logits_c_stride", "dlogits_batch_stride", "dlogits_c_stride", "target_batch_stride", "logits", "target", "loss", "coef",
        "workspace", "workspace_bytes", "grad_out", "dlogits"]
    assert ctypes.sizeof(P) == 144 and dict(P._fields_)["eps"] is ctypes.c_float
    text = open(HEADER).read()
    assert "#ifndef VIVIM_HIP_EXT_H" in text and '#include "vivim_hip.h"' in text


def test_the_library_exports_the_three_symbols():
    L = _lib.lib()
    for n in NAMES:
        fn = getattr(L, n)
        assert fn.argtypes[0] is ctypes.POINTER(P) and fn.restype is _lib.ALL_ENTRY_POINTS[n].restype


def test_layout_matches_the_c_compiler(tmp_path):
    layout_matches_c("vivim_hip_ext.h", "vivim_structure_loss_params", P, tmp_path)


# ---- refusals

def _good(**over):
    p = P()
    p.struct_bytes = ctypes.sizeof(P)
    p.batch, p.classes, p.height, p.width, p.itype, p.ttype, p.first_class, p.eps = 2, 3, 33, 47, _lib.BF16, 0, 0, 1e-6
    p.logits_batch_stride, p.logits_c_stride, p.target_batch_stride = 3 * 33 * 47, 33 * 47, 33 * 47
    p.dlogits_batch_stride, p.dlogits_c_stride = 3 * 33 * 47, 33 * 47
    p.logits = p.target = p.loss = p.coef = p.workspace = p.grad_out = p.dlogits = PTR
    for k, v in over.items():
        setattr(p, k, v)
    if "workspace_bytes" not in over:
        p.workspace_bytes = _lib.lib().vivim_structure_loss_workspace_bytes(p)
    return p


@pytest.mark.parametrize("name", NAMES[1:])
def test_refusals_before_any_launch(name):
    fn = name[len("vivim_"):]
    bwd = name.endswith("bwd")
    assert f"{fn}: params is NULL" in _refused(name, None)
    assert "struct_bytes = 0, this library's vivim_structure_loss_params has 144" in _refused(name, _good(struct_bytes=0))
    assert "struct_bytes = 152" in _refused(name, _good(struct_bytes=152))
    assert "itype = 7" in _refused(name, _good(itype=7, workspace_bytes=1 << 20))
    assert "ttype = 2" in _refused(name, _good(ttype=2))
    for field in ("batch", "classes", "height", "width"):
        for v in (0, -3):
            assert f"{field} = {v}" in _refused(name, _good(**{field: v, "workspace_bytes": 1 << 20})), field
    assert "9 classes: the kernels are built for 1 to 8 classes" in _refused(name, _good(classes=9, workspace_bytes=1 << 20), code=2)
    for v in (-1, 256):
        assert f"first_class = {v}" in _refused(name, _good(first_class=v))
    for field, align in (("logits", 2), ("target", 8)):
        assert f"{field} at (nil)" in _refused(name, _good(**{field: None}))
        assert f"{field} at 0x1001: need a {align}-byte aligned pointer" in _refused(name, _good(**{field: PTR + 1}))
    for over in (dict(height=1 << 16, width=1 << 15), dict(height=46341, width=46341), dict(batch=1 << 30, height=64, width=64)):
        assert "the index range overflows int32" in _refused(name, _good(workspace_bytes=1 << 40, **over))
    if not bwd:
        assert "loss at (nil)" in _refused(name, _good(loss=None))
        assert "loss at 0x1002" in _refused(name, _good(loss=PTR + 2))
        assert "coef at 0x1002" in _refused(name, _good(coef=PTR + 2))
        need = _good().workspace_bytes
        assert need == 4 * 4 * 2 * 2 * 3                       # bf16: 32-row tiles, two down and one across, 4 floats per channel
        assert f"workspace of {need} bytes at (nil)" in _refused(name, _good(workspace=None))
        assert f"workspace of {need - 4} bytes at 0x1000" in _refused(name, _good(workspace_bytes=need - 4))
        assert "need a 8-byte aligned one of vivim_structure_loss_workspace_bytes() = %d" % need in _refused(name, _good(workspace=PTR + 4))
        assert "workspace of -1 bytes" in _refused(name, _good(workspace_bytes=-1))
    else:
        for field in ("coef", "grad_out", "dlogits"):
            assert f"{field} at (nil)" in _refused(name, _good(**{field: None}))
            assert f"{field} at 0x1001" in _refused(name, _good(**{field: PTR + 1}))


def test_workspace_bytes_depend_on_the_sizes_alone_and_grow_with_them():
    L = _lib.lib()
    q = L.vivim_structure_loss_workspace_bytes
    assert q(None) == 0
    for bad in (dict(struct_bytes=0), dict(batch=0), dict(classes=0), dict(classes=9), dict(height=0), dict(width=-1), dict(itype=3)):
        assert q(_good(workspace_bytes=0, **bad)) == 0, bad
    base = dict(batch=2, classes=3, height=33, width=47, workspace_bytes=0)
    for itype in (_lib.F32, _lib.F16, _lib.BF16):
        prev = q(_good(itype=itype, **base))
        assert prev > 0 and prev % 16 == 0
        assert prev == q(_good(itype=itype, logits=None, target=None, first_class=99, **base))       # no pointer, no label is read
        for field in ("batch", "classes", "height", "width"):
            last = prev
            for v in range(base[field], base[field] + 140, 7 if field in ("height", "width") else 1):
                if field == "classes" and v > 8:
                    break
                cur = q(_good(itype=itype, **dict(base, **{field: v})))
                assert cur >= last > 0, (field, v)
                last = cur
            assert last > prev, field
    assert q(_good(itype=_lib.F32, **base)) == 16 * 2 * 3 * 3 and q(_good(itype=_lib.F16, **base)) == 16 * 2 * 2 * 3


# ---- the eager functions

def formula64(logits, targets, first, eps):
    """The definition, per pixel and per class in fp64: k by counting, w = 1 + 5 |k / 961 - m|, the four sums, the loss."""
    x = logits.double()
    N, C, H, W = x.shape
    total = 0.0
    for c in range(C):
        m = (targets == c + first)[:, None].double()
        k = F.conv2d(F.pad(m, (15, 15, 15, 15)), torch.ones(1, 1, 31, 31, dtype=torch.float64))
        w = 1 + 5 * (k / 961 - m).abs()
        xc = x[:, c:c + 1]
        s = torch.sigmoid(xc)
        bce = xc.clamp_min(0) - xc * m + torch.log1p(torch.exp(-xc.abs()))
        sums = [(w * v).sum(dim=(1, 2, 3)) for v in (torch.ones_like(m), bce, s * m, s + m - s * m)]
        total = total + (sums[1] / sums[0] + 1 - (sums[2] + eps) / (sums[3] + eps)).sum()
    return total / (N * C)


@pytest.mark.parametrize("case, content", [("binary", "mixed"), ("odd", "mixed"), ("odd", "holes"), ("c5", "solid"), ("wide", "mixed")])
def test_eager_functions_are_the_formula(case, content):
    (N, C, H, W), first, eps = sc.SHAPES[case]
    logits, targets = sc.make_case(case, torch.float32, 4.0, seed=1, content=content)
    if content == "mixed":
        assert int((targets[0] == first + C - 1).sum()) == 0                                   # a class absent from an image
    if content == "holes":
        assert int(((targets < 0) | (targets >= C)).sum()) > 0                                 # labels outside [0, C)
    x = logits.double()
    want = formula64(x, targets, first, eps)
    if first == 0:
        got = sl.multiclass_structure_loss(x, targets, C)
        assert inspect.signature(sl.multiclass_structure_loss).parameters["eps"].default == eps
    else:
        got = sl.structure_loss(x, (targets == 1)[:, None].double())
        assert inspect.signature(sl.structure_loss).parameters["eps"].default == eps
    assert got.dtype == torch.float64 and abs(float(got) - float(want)) <= 1e-12 * abs(float(want))
    ref, _ = sc.ref64(logits, targets, first, eps)
    assert abs(float(ref) - float(want)) <= 1e-12 * abs(float(want))                           # the shared fp64 reference, likewise
    # 16-bit logits are widened to fp32, as recall_focused_loss does
    half = sl.multiclass_structure_loss(logits.bfloat16(), targets, C, eps) if first == 0 else None
    assert half is None or half.dtype == torch.float32


@pytest.mark.parametrize("name", ["structloss_binary", "structloss_c3", "structloss_c5"])
def test_eager_functions_against_the_references_own_output(name):
    """The fixtures are the reference's functions on fp64 logits.  Those build their mask and weight map in fp32 (`.float()` one-hot,
    avg_pool2d of it), so a weight carries a relative error of up to 2^-24 = 6e-8 that the fp64 evaluation here does not have: the
    allowance is 1e-6 of the loss and, norm-wise, of the gradient -- an order above that, five below any real difference."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    x = torch.from_numpy(z["logits"]).requires_grad_(True)
    assert x.dtype == torch.float64
    if "mask" in z.files:
        assert tuple(x.shape) == (2, 1, 9, 11) and float(z["eps"]) == 1.0
        mask = torch.from_numpy(z["mask"])
        loss = sl.structure_loss(x, mask)
        # what the binary recipe computes as written (`reduce='none'`): the weighted IoU term plus the unweighted mean BCE
        with torch.no_grad():
            plain = F.binary_cross_entropy_with_logits(x, mask)
            w = 1 + 5 * (F.avg_pool2d(mask, 31, 1, 15) - mask).abs()
            wbce = ((w * F.binary_cross_entropy_with_logits(x, mask, reduction="none")).sum(dim=(2, 3)) / w.sum(dim=(2, 3))).mean()
        assert abs(float(loss.detach() - wbce + plain) - float(z["loss_as_written"])) <= 1e-6 * float(z["loss_as_written"])
    else:
        C = x.shape[1]
        assert tuple(x.shape) in ((2, 3, 33, 47), (1, 5, 40, 31)) and float(z["eps"]) == 1e-6
        loss = sl.multiclass_structure_loss(x, torch.from_numpy(z["targets"]), C)
    loss.backward()
    want = torch.from_numpy(z["dlogits"])
    assert abs(float(loss.detach()) - float(z["loss"])) <= 1e-6 * float(z["loss"])
    assert float((x.grad - want).norm() / want.norm()) <= 1e-6


# ---- the kernels' arithmetic, restated in fp32

@pytest.mark.parametrize("case", list(sc.SHAPES))
def test_restated_arithmetic_meets_the_gpu_bounds(case):
    """Every input of tests/test_gpu_structure_loss.py's grid through structure_loss_cases.restate32 and the same checks: the bounds
    are reachable by fp32 arithmetic of the kernels' form.  Prints the figure FLOOR is derived from."""
    (N, C, H, W), first, eps = sc.SHAPES[case]
    worst = worst_eager = 0.0
    for dt, dtype in sc.DTYPES.items():
        for scale in sc.SCALES:
            for content in sc.CONTENTS:
                logits, targets = sc.make_case(case, dtype, scale, content=content)
                tag = f"restate32[{case} {dt} scale {scale:g} {content}]"
                wide = logits.float()
                want_loss, want = sc.ref64(wide, targets, first, eps)
                loss, grad = sc.restate32(wide, targets, first, eps)
                _, eager = sc.eager32(wide, targets, C, first, eps)
                sc.check_loss(tag, loss, want_loss)
                sc.check_norm(tag, grad, want, torch.float32)
                e, ee = sc.check_elementwise(tag, grad, eager, want)
                worst, worst_eager = max(worst, e), max(worst_eager, ee)
                if dtype != torch.float32:
                    sc.check_norm(tag, grad.to(dtype), want, dtype)
                    sc.check_one_rounding(tag, grad.to(dtype), grad, dtype)
    print(f"{case}: worst max|err| / max|want| of the restatement {worst:.3e}, of the eager composition {worst_eager:.3e}; "
          f"floor {sc.FLOOR:.1e}")
    assert 4 * worst <= sc.FLOOR


def test_restated_arithmetic_under_the_loss_scale():
    """fp16 logits, upstream 65536: multiplied in fp32 before the one rounding, no gradient that fp16 can hold is flushed."""
    (N, C, H, W), first, eps = sc.SHAPES["odd"]
    logits, targets = sc.make_case("odd", torch.float16, 8.0, seed=4)
    _, want = sc.ref64(logits, targets, first, eps, upstream=65536.0)
    _, grad = sc.restate32(logits, targets, first, eps, upstream=65536.0)
    sc.check_norm("restate32[65536]", grad.half(), want, torch.float16)
    assert bool((grad.half()[want.half() != 0] != 0).all())


def test_window_counts_are_the_average_pool():
    g = torch.Generator().manual_seed(0)
    for H, W in ((5, 7), (31, 31), (33, 47), (20, 130)):
        m = torch.rand(2, 2, H, W, generator=g) < 0.5
        k = sc.window_counts(m)
        pooled = F.avg_pool2d(m.double(), kernel_size=31, stride=1, padding=15) * 961
        assert k.dtype == torch.int64 and torch.equal(k, pooled.round().long()) and float((pooled - pooled.round()).abs().max()) < 1e-9


# ---- gating and the criterion keyword

def test_supported_says_no_on_the_cpu_and_the_fused_names_run_the_eager_loss():
    logits, targets = sc.make_case("odd", torch.float32, 4.0, seed=2)
    assert not sl.supported(logits, targets, 3)
    a, b = logits.clone().requires_grad_(True), logits.clone().requires_grad_(True)
    la, lb = sl.multiclass_structure_loss_fused(a, targets, 3), sl.multiclass_structure_loss(b, targets, 3)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
    pred, labels = sc.make_case("binary", torch.float32, 4.0, seed=2)
    mask = (labels == 1)[:, None].float()
    assert sl._binary_labels(pred, mask) is None
    assert torch.equal(sl.structure_loss_fused(pred, mask), sl.structure_loss(pred, mask))
    assert torch.equal(sl.structure_loss_fused(pred, mask * 0.5), sl.structure_loss(pred, mask * 0.5))     # a soft mask: eager
    import vivim_amd
    assert vivim_amd.multiclass_structure_loss_fused is sl.multiclass_structure_loss_fused
    assert vivim_amd.structure_loss_fused is sl.structure_loss_fused and vivim_amd.multiclass_structure_loss is sl.multiclass_structure_loss


class _Stub(torch.nn.Module):
    def __init__(self, C):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, C, 1)

    def forward(self, clip):
        return self.conv(clip.flatten(0, 1))


def test_the_criterion_keyword_is_trailing_and_selects_the_loss():
    from vivim_amd import train_step as ts
    for fn in (ts.train_step, ts.eval_step):
        names = list(inspect.signature(fn).parameters)
        assert names[-1] == "criterion" and inspect.signature(fn).parameters["criterion"].default == "recall_focused"
    clip, onehot = ts.synthetic_batch(1, 2, 12, 3, "cpu", seed=3)
    target = onehot.argmax(dim=2).view(2, 12, 12)
    torch.manual_seed(0)
    model = _Stub(3)
    with torch.no_grad():
        logits = model(clip)
    want = {"recall_focused": ts.recall_focused_loss(logits, target, 3), "structure": sl.multiclass_structure_loss(logits, target, 3)}
    for fused in (False, True):                                    # CPU tensors: the fused route is the eager loss, bit for bit
        assert torch.equal(ts.eval_step(model, clip, onehot, 3, amp_dtype=torch.float32, fused_loss=fused), want["recall_focused"])
        for criterion in want:
            got = ts.eval_step(model, clip, onehot, 3, amp_dtype=torch.float32, fused_loss=fused, criterion=criterion)
            assert torch.equal(got, want[criterion]), (fused, criterion)
    with pytest.raises(ValueError, match="criterion 'dice'"):
        ts.eval_step(model, clip, onehot, 3, amp_dtype=torch.float32, criterion="dice")
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    before = [p.detach().clone() for p in model.parameters()]
    loss = ts.train_step(model, opt, clip, onehot, 3, amp_dtype=torch.float32, fused_loss=True, criterion="structure")
    assert torch.equal(loss, want["structure"]) and any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
