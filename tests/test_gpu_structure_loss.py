"""GPU: the fused structure loss (vivim_amd/structure_loss.py, csrc/structure_loss.hip) against the reference's formula in fp64 on
the CPU from the same inputs (structure_loss_cases.ref64), and against the fixtures the reference's own functions produced.

Cases, bounds and the floor are structure_loss_cases.py's, the same that tests/test_abi_structure_loss.py holds the fp32 restatement
of the kernels' arithmetic to: loss <= 1e-5 relative; dlogits < 1e-3 norm-wise; 16-bit dlogits within one rounding of the fp32 value;
elementwise |err(fused)| <= 2 * |err(eager fp32 on the same inputs)| + floor * max|want|.  The floor: the restatement's measured worst
max|err| / max|want| over these inputs is 3.62e-7, the chosen floor 4 x that, rounded up: 1.5e-6.  The eager composition's errors
are logged next to ours (tests/conftest.py's parity log), not asserted."""
import os

import numpy as np
import pytest
import torch

import structure_loss_cases as sc
from conftest import _PARITY_LOG, GOLDEN, rel_err
from vivim_amd import _lib

pytestmark = pytest.mark.gpu


def _log(name, dtype, got, want, test):
    e = rel_err(got.double(), want.double())
    mx = float((got.double().cpu() - want.double().cpu()).abs().max())
    try:
        os.makedirs(os.path.dirname(_PARITY_LOG), exist_ok=True)
        with open(_PARITY_LOG, "a") as f:
            f.write(f"{test}\t{name}\t{str(dtype).replace('torch.', '')}\tshape={tuple(got.shape)}\trel_err={e:.3e}\tmax_abs={mx:.3e}\n")
    except OSError:
        pass
    return e


def run_fused(logits, targets, first, eps, upstream=None):
    """-> (loss, dlogits) of the fused route for device tensors; the logits keep the strides of a view."""
    from vivim_amd import structure_loss as sl
    C = logits.shape[1]
    x = logits.detach().requires_grad_(True)
    if first == 0:
        assert sl.supported(x, targets, C)
        loss = sl.multiclass_structure_loss_fused(x, targets, C, eps)
    else:
        mask = (targets == first)[:, None]
        assert sl._binary_labels(x, mask) is not None
        loss = sl.structure_loss_fused(x, mask, eps)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.grad_fn is not None
    if upstream is None:
        loss.backward()
    else:
        upstream(loss)
    assert x.grad.dtype == logits.dtype and x.grad.is_contiguous()
    return loss.detach(), x.grad


def check_case(tag, logits, targets, first, eps, test, want=None):
    """Every bound of structure_loss_cases for one input on the device -> (loss, dlogits)."""
    dtype, C = logits.dtype, logits.shape[1]
    want_loss, want_grad = want or sc.ref64(logits, targets, first, eps)
    loss, grad = run_fused(logits, targets, first, eps)
    sc.check_loss(tag, loss, want_loss)
    sc.check_norm(tag, grad, want_grad, dtype)
    _log(tag + ".dlogits", dtype, grad.cpu(), want_grad.to(dtype), test)
    wide = logits.float()
    if dtype == torch.float32:
        g32 = grad
    else:
        loss32, g32 = run_fused(wide, targets, first, eps)          # the same values through the fp32 instantiation
        sc.check_loss(tag + " (widened)", loss32, want_loss)
        sc.check_one_rounding(tag, grad, g32, dtype)
    _, eager = sc.eager32(wide, targets, C, first, eps)              # the eager fp32 composition on the same inputs, on the device
    _log(tag + ".dlogits(eager)", torch.float32, eager.cpu(), want_grad, test)
    sc.check_elementwise(tag, g32, eager, want_grad)
    return loss, grad


@pytest.mark.parametrize("dt", list(sc.DTYPES))
@pytest.mark.parametrize("case", list(sc.SHAPES))
def test_parity_grid(cuda, case, dt, request):
    (N, C, H, W), first, eps = sc.SHAPES[case]
    for scale in sc.SCALES:
        logits, targets = sc.make_case(case, sc.DTYPES[dt], scale)
        assert int((targets[0] == first + C - 1).sum()) == 0                            # a class absent from image 0
        check_case(f"structure_loss[{case} {N}x{C}x{H}x{W} {dt} scale {scale:g}]", logits.to(cuda), targets.to(cuda), first, eps,
                   request.node.name)


@pytest.mark.parametrize("content", ("solid", "holes"))
@pytest.mark.parametrize("case", ("binary", "odd", "wide"))
def test_label_content(cuda, case, content, request):
    """An image made of one class only; labels outside the classes, which belong to no class whatever their value."""
    (N, C, H, W), first, eps = sc.SHAPES[case]
    for dtype in (torch.float32, torch.float16):
        logits, targets = sc.make_case(case, dtype, 8.0, seed=3, content=content)
        x, t = logits.to(cuda), targets.to(cuda)
        loss, grad = check_case(f"structure_loss[{case} {content}]", x, t, first, eps, request.node.name)
        if content == "holes":
            outside = (t < first) | (t >= first + C) if C > 1 else (t != 0) & (t != 1)
            assert int(outside.sum()) > 0
            for other in (255, -1, first + C, 2 ** 32 + first, -2 ** 40):
                loss_o, grad_o = run_fused(x, t.masked_fill(outside, other), first, eps)
                assert torch.equal(loss_o, loss) and torch.equal(grad_o, grad), other


@pytest.mark.parametrize("case", ("binary", "odd", "c8", "wide"))
def test_uint8_targets(cuda, case, request):
    (N, C, H, W), first, eps = sc.SHAPES[case]
    for dtype in (torch.float32, torch.bfloat16):
        logits, targets = sc.make_case(case, dtype, 8.0, seed=2)
        x, t64 = logits.to(cuda), targets.to(cuda)
        t8 = t64.to(torch.uint8)
        if first == 0:
            from vivim_amd import structure_loss as sl
            x8 = x.detach().requires_grad_(True)
            assert sl.supported(x8, t8, C)
            loss = sl.multiclass_structure_loss_fused(x8, t8, C, eps)
            loss.backward()
            got = (loss.detach(), x8.grad)
        else:
            got = run_fused(x, t8, first, eps)
        ref = check_case(f"structure_loss[uint8 {case}]", x, t64, first, eps, request.node.name)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


@pytest.mark.parametrize("dt", list(sc.DTYPES))
@pytest.mark.parametrize("offset", (0, 1))
def test_channel_slice_views(cuda, dt, offset, request):
    """Logits as a channel slice of a wider tensor (batch and channel strides differ from the packed ones); with offset 1 the same
    view starts one element into its storage, which no 16-byte vector can reach.  W = 48 is a whole number of vectors, so the packed
    tensor and the offset-0 view take the vector path."""
    dtype = sc.DTYPES[dt]
    N, C, H, W = 2, 3, 33, 48
    g = torch.Generator().manual_seed(11)
    packed = (torch.randn(N, C, H, W, generator=g) * 8).to(dtype).to(cuda)
    targets = torch.randint(0, C, (N, H, W), generator=g).to(cuda)
    flat = torch.full((N * (C + 3) * H * W + offset,), float("nan"), dtype=dtype, device=cuda)
    wide = flat[offset:].view(N, C + 3, H, W)
    view = wide[:, 2:2 + C]
    view.copy_(packed)
    assert view.stride() == ((C + 3) * H * W, H * W, W, 1) and (view.data_ptr() % 16 == 0) == (offset == 0)
    want = sc.ref64(packed, targets, 0, 1e-6)
    loss, grad = check_case(f"structure_loss[slice offset {offset}]", view, targets, 0, 1e-6, request.node.name, want=want)
    loss_p, grad_p = run_fused(packed, targets, 0, 1e-6)
    assert torch.equal(loss, loss_p) and torch.equal(grad, grad_p)          # vector or element accesses: the same arithmetic
    assert bool(torch.isnan(wide[:, :2]).all()) and bool(torch.isnan(wide[:, 2 + C:]).all())


@pytest.mark.parametrize("name", ["structloss_binary", "structloss_c3", "structloss_c5"])
def test_against_the_references_own_output(cuda, name):
    """The fixtures (the reference's functions on fp64 logits), their logits rounded to fp32: loss and gradient move by the rounding of
    the inputs as well, so the reference here is the fixture's loss to 1e-5 and its gradient norm-wise to 1e-3 -- the project's bounds --
    with the fp64 formula on the rounded logits in between, to which the usual checks apply."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    logits = torch.from_numpy(z["logits"]).float()
    if "mask" in z.files:
        targets, first, eps = torch.from_numpy(z["mask"])[:, 0].long(), 1, 1.0
    else:
        targets, first, eps = torch.from_numpy(z["targets"]), 0, 1e-6
    loss, grad = check_case(f"structure_loss[{name}]", logits.to(cuda), targets.to(cuda), first, eps, name)
    assert abs(float(loss) - float(z["loss"])) <= 1e-5 * float(z["loss"])
    want = torch.from_numpy(z["dlogits"])
    assert float((grad.cpu().double() - want).norm() / want.norm()) < 1e-3


def test_upstream_gradient(cuda, request):
    (N, C, H, W), first, eps = sc.SHAPES["odd"]
    logits, targets = sc.make_case("odd", torch.float32, 8.0, seed=4)
    x, t = logits.to(cuda), targets.to(cuda)
    _, want = sc.ref64(logits, targets, first, eps, upstream=3.0)
    _, grad = run_fused(x, t, first, eps, upstream=lambda l: (3 * l).backward())
    sc.check_norm("structure_loss[3 * loss]", grad, want, torch.float32)
    # fp16 logits under the train step's loss scale: multiplied in fp32 before the one rounding, so nothing is flushed
    logits, targets = sc.make_case("odd", torch.float16, 8.0, seed=4)
    x, t = logits.to(cuda), targets.to(cuda)
    _, want = sc.ref64(logits, targets, first, eps, upstream=65536.0)
    for up in (lambda l: l.backward(torch.tensor(65536.0, device=cuda)), lambda l: (l * 65536.0).backward()):
        _, grad = run_fused(x, t, first, eps, upstream=up)
        sc.check_norm("structure_loss[65536]", grad, want, torch.float16)
        assert bool((grad.cpu()[want.half() != 0] != 0).all())
    _, g32 = run_fused(x.float(), t, first, eps, upstream=lambda l: l.backward(torch.tensor(65536.0, device=cuda)))
    sc.check_one_rounding("structure_loss[65536]", grad, g32, torch.float16)


@pytest.mark.parametrize("dt", list(sc.DTYPES))
def test_repeatable_bits(cuda, dt):
    """No atomics: a second call, a call on a side stream and a call under use_deterministic_algorithms give the same bits."""
    (N, C, H, W), first, eps = sc.SHAPES["c8"]
    logits, targets = sc.make_case("c8", sc.DTYPES[dt], 8.0, seed=7)
    x, t = logits.to(cuda), targets.to(cuda)
    loss0, grad0 = run_fused(x, t, first, eps)
    loss1, grad1 = run_fused(x, t, first, eps)
    assert torch.equal(loss0, loss1) and torch.equal(grad0, grad1)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        loss2, grad2 = run_fused(x, t, first, eps)
    side.synchronize()
    torch.cuda.current_stream(cuda).wait_stream(side)
    assert torch.equal(loss0, loss2) and torch.equal(grad0, grad2)
    torch.use_deterministic_algorithms(True)
    try:
        loss3, grad3 = run_fused(x, t, first, eps)
    finally:
        torch.use_deterministic_algorithms(False)
    assert torch.equal(loss0, loss3) and torch.equal(grad0, grad3)


def test_no_grad_passes_no_coef_and_saves_nothing(cuda, monkeypatch):
    from vivim_amd import structure_loss as sl
    (N, C, H, W), first, eps = sc.SHAPES["odd"]
    logits, targets = sc.make_case("odd", torch.bfloat16, 8.0, seed=8)
    x, t = logits.to(cuda), targets.to(cuda)
    loss0, _ = run_fused(x, t, first, eps)
    seen = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, P, stream: (seen.append((name, P.coef)), real_call(name, P, stream))[1])
    xg = x.detach().requires_grad_(True)
    with torch.no_grad():
        loss1 = sl.multiclass_structure_loss_fused(xg, t, C)
    loss2 = sl.multiclass_structure_loss_fused(x.detach(), t, C)            # logits that want no gradient
    assert seen == [("vivim_structure_loss_fwd", None)] * 2                  # coef = NULL: the forward alone
    for loss in (loss1, loss2):
        assert torch.equal(loss0, loss) and not loss.requires_grad and loss.grad_fn is None
    with pytest.raises(RuntimeError):
        loss1.backward()


def test_fallbacks_return_the_eager_loss(cuda):
    from vivim_amd import structure_loss as sl
    g = torch.Generator().manual_seed(9)
    l9 = torch.randn(2, 9, 8, 8, generator=g).to(cuda)
    t9 = torch.randint(0, 9, (2, 8, 8), generator=g).to(cuda)
    assert not sl.supported(l9, t9, 9)                                       # more than 8 classes
    assert torch.equal(sl.multiclass_structure_loss_fused(l9, t9, 9), sl.multiclass_structure_loss(l9, t9, 9))
    logits, targets = (v.to(cuda) for v in sc.make_case("odd", torch.float32, 2.0, seed=9))
    cl = logits.contiguous(memory_format=torch.channels_last)
    assert cl.stride(3) != 1 and not sl.supported(cl, targets, 3)           # another layout
    assert not sl.supported(logits.double(), targets, 3) and not sl.supported(logits, targets.int(), 3)     # other dtypes
    a, b = cl.detach().requires_grad_(True), cl.detach().requires_grad_(True)
    la, lb = sl.multiclass_structure_loss_fused(a, targets, 3), sl.multiclass_structure_loss(b, targets, 3)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
    pred, labels = (v.to(cuda) for v in sc.make_case("binary", torch.float32, 2.0, seed=9))
    soft = (labels == 1)[:, None].float() * 0.5                              # a mask that is not exactly {0, 1}
    assert sl._binary_labels(pred, soft) is None and sl._binary_labels(pred, soft * 2) is not None
    assert torch.equal(sl.structure_loss_fused(pred, soft), sl.structure_loss(pred, soft))


class _Stub(torch.nn.Module):
    """(B, nf, 3, H, W) -> (B * nf, C, H, W) through a 1 x 1 convolution: what train_step needs of a model."""

    def __init__(self, C):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, C, 1)

    def forward(self, clip):
        return self.conv(clip.flatten(0, 1))


def test_train_step_end_to_end(cuda, monkeypatch):
    from vivim_amd import train_step as ts
    calls = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, P, stream: (calls.append(name), real_call(name, P, stream))[1])
    clip, onehot = ts.synthetic_batch(2, 3, 40, 3, cuda, seed=11)
    out = {}
    for fused in (True, False):
        torch.manual_seed(12)
        model = _Stub(3).to(cuda)
        opt = ts.make_optimizer(model, lr=1e-2)
        del calls[:]
        losses = [float(ts.train_step(model, opt, clip, onehot, 3, amp_dtype=torch.float32, fused_loss=fused, criterion="structure"))
                  for _ in range(3)]
        names = [n for n in calls if "loss" in n]
        assert names == (["vivim_structure_loss_fwd", "vivim_structure_loss_bwd"] * 3 if fused else [])
        assert all(np.isfinite(v) for v in losses) and all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())
        out[fused] = (losses, torch.cat([p.detach().flatten() for p in model.parameters()]))
        loss = ts.eval_step(model, clip, onehot, 3, amp_dtype=torch.float32, fused_loss=fused, criterion="structure")
        assert bool(torch.isfinite(loss)) and not loss.requires_grad
    for a, b in zip(out[True][0], out[False][0]):
        assert abs(a - b) <= 1e-5 * abs(b), (out[True][0], out[False][0])
    e = rel_err(out[True][1], out[False][1])
    assert e < 1e-3, e
