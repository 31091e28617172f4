"""GPU: the fused recall-focused loss (vivim_amd/seg_loss.py, csrc/seg_loss.hip) against an fp64 restatement of the loss formulas
(multiclass_training_folds.py:218-255, 339-423) written out below -- train_step.recall_focused_loss casts to fp32 and cannot
serve as the reference.

Tolerances.  Loss: relative error <= 1e-5 (fp32 roundoff 6e-8 x a few ulp per transcendental + log2(n) for the tree sums is about
1e-6; every grid shape is small enough that one dropped pixel moves the loss by far more).  dlogits, against fp64 autograd ROUNDED
TO THE LOGITS' DTYPE: norm-wise < 1e-3, and elementwise |err| <= rtol * |want| + 1e-3 * max|want| with rtol = 1e-3 for fp32 and two
ulp of the dtype for fp16 / bf16 (2^-9, 2^-6: a rounding-boundary flip between two fp32-accurate values); a wrong tail pixel errs
by O(max|want|), a thousand times the allowance.  The eager fp32 composition's errors are logged next to ours, not asserted."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import _PARITY_LOG, rel_err
from vivim_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
ITYPE = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}
RTOL = {torch.float32: 1e-3, torch.float16: 2.0 ** -9, torch.bfloat16: 2.0 ** -6}
SCALES = (1.0, 4.0, 8.0, 30.0)


def _alpha(C):
    return (0.05, 0.475, 0.475) if C == 3 else tuple([1.0 / C] * C)


def ref64(logits, targets, C, alpha=None, upstream=1.0):
    """fp64 loss and d(upstream * loss)/dlogits by autograd.  The one-hot rows come from comparisons, so a label outside [0, C) has
    an all-zero row."""
    x = logits.detach().double().requires_grad_(True)
    probs = F.softmax(x, dim=1)
    onehot = (targets.long()[:, None] == torch.arange(C, device=x.device)[None, :, None, None]).double()
    a = torch.tensor(alpha or _alpha(C), dtype=torch.float64, device=x.device)[None, :, None, None]
    weight = onehot * (1 - probs) ** 2 + (1 - onehot) * probs ** 2
    bce = -onehot * torch.log(probs + 1e-6) - (1 - onehot) * torch.log(1 - probs + 1e-6)
    focal = (a * weight * bce).mean(dim=(0, 2, 3)).sum()
    tp = (probs * onehot).sum(dim=(2, 3))
    fp = (probs * (1 - onehot)).sum(dim=(2, 3))
    fn = ((1 - probs) * onehot).sum(dim=(2, 3))
    tv = (tp + 1e-6) / (tp + 0.3 * fp + 0.7 * fn + 1e-6)
    loss = 0.4 * focal + 0.6 * (1 - tv.mean(dim=0)).mean()
    (upstream * loss).backward()
    return loss.detach(), x.grad


def make_case(cuda, shape, dtype, scale, seed=0, ttype=torch.int64):
    """Logits randn * scale rounded to the dtype first; image 0 has its last class relabelled, so one class is absent there."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed * 1000 + N * 100 + C * 10 + H)
    logits = (torch.randn(N, C, H, W, generator=g) * scale).to(dtype).to(cuda)
    targets = torch.randint(0, C, (N, H, W), generator=g)
    targets[0][targets[0] == C - 1] = 0
    return logits, targets.to(ttype).to(cuda)


def _log(name, dtype, got, want, test):
    e = rel_err(got.double(), want.double())
    mx = float((got.double() - want.double()).abs().max())
    try:
        os.makedirs(os.path.dirname(_PARITY_LOG), exist_ok=True)
        with open(_PARITY_LOG, "a") as f:
            f.write(f"{test}\t{name}\t{str(dtype).replace('torch.', '')}\tshape={tuple(got.shape)}\trel_err={e:.3e}\tmax_abs={mx:.3e}\n")
    except OSError:
        pass
    return e


def check_grad(name, got, want64, dtype, test):
    assert got.dtype == dtype and got.is_contiguous()
    want = want64.to(dtype).double()                       # fp64 autograd rounded to the logits' dtype
    g = got.double()
    assert torch.isfinite(g).all(), f"{name}: non-finite gradient"
    e = _log(name, dtype, g, want, test)
    print(f"{test} {name} {dtype}: dlogits norm-wise {e:.3e}, max|err| / max|want| "
          f"{float((g - want).abs().max() / want.abs().max()):.3e}")
    assert e < 1e-3, f"{name}: rel-err {e:.3e} >= 1e-3"
    allow = RTOL[dtype] * want.abs() + 1e-3 * want.abs().max()
    bad = (g - want).abs() > allow
    assert not bool(bad.any()), (f"{name} ({dtype}): {int(bad.sum())} of {bad.numel()} elements outside the allowance, worst "
                                 f"{float(((g - want).abs() - allow).max()):.3e} over it, first at {bad.nonzero()[0].tolist()}")


def check_loss(name, got, want64, test):
    assert got.dtype == torch.float32 and got.dim() == 0
    e = abs(float(got) - float(want64)) / abs(float(want64))
    print(f"{test} {name}: loss {float(got):.8f} want {float(want64):.8f} rel {e:.3e}")
    assert e <= 1e-5, f"{name}: loss {float(got)!r} against {float(want64)!r}: relative error {e:.3e} > 1e-5"
    return e


def run_fused(logits, targets, C, upstream=None, alpha=None):
    from vivim_amd import seg_loss
    assert seg_loss.supported(logits, targets, C, 2.0)
    x = logits.detach().requires_grad_(True)                # keeps the strides of a view
    loss = seg_loss.recall_focused_loss_fused(x, targets, C, alpha=alpha)
    if upstream is None:
        loss.backward()
    else:
        upstream(loss)
    return loss.detach(), x.grad


def _blocks_per_image(N, C, pixels, dtype):
    P = _lib.SegLossParams()
    P.batch, P.classes, P.pixels, P.itype = N, C, pixels, ITYPE[dtype]
    b = _lib.lib().vivim_seg_loss_workspace_bytes(ctypes.byref(P))
    assert b > 0 and b % (4 * N * (3 * C + 1)) == 0
    return b // (4 * N * (3 * C + 1))


def _ragged_shape(dtype, N=1, C=3, W=53):
    """The smallest (N, C, H, 53) that the library cuts into at least 3 workgroups per image: W is odd, so the last one is ragged."""
    H = 1
    while _blocks_per_image(N, C, H * W, dtype) < 3:
        H += 1
        assert H < 4096
    return (N, C, H, W)


def _strided_shape(dtype, N=1, C=2, W=257):
    """Just past the cap on workgroups per image: every workgroup goes round its grid-stride loop, the first ones twice."""
    cap = _blocks_per_image(N, C, 1 << 28, dtype)
    per_block = 1
    while _blocks_per_image(N, C, per_block + 1, dtype) < 2:
        per_block *= 2
    H = (cap * per_block) // W + 3
    assert _blocks_per_image(N, C, H * W, dtype) == cap and cap * per_block < H * W < (cap + 1) * per_block
    return (N, C, H, W)


GRID = {"35px": (2, 3, 5, 7), "vec": (3, 3, 16, 24), "c2": (2, 2, 8, 8), "c5": (1, 5, 9, 11), "c8": (2, 8, 6, 10),
        "ragged": _ragged_shape}


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", list(GRID))
def test_parity_grid(cuda, case, dt, request):
    dtype = DTYPES[dt]
    shape = GRID[case](dtype) if callable(GRID[case]) else GRID[case]
    from vivim_amd.train_step import recall_focused_loss
    N, C, H, W = shape
    for scale in SCALES:
        logits, targets = make_case(cuda, shape, dtype, scale)
        assert int((targets[0] == C - 1).sum()) == 0
        want_loss, want_grad = ref64(logits, targets, C)
        loss, grad = run_fused(logits, targets, C)
        name = f"seg_loss[{case} {N}x{C}x{H}x{W} scale {scale:g}]"
        check_loss(name, loss, want_loss, request.node.name)
        check_grad(name + ".dlogits", grad, want_grad, dtype, request.node.name)
        # the eager fp32 composition on the same inputs: recorded, not asserted
        x = logits.detach().requires_grad_(True)
        le = recall_focused_loss(x, targets, C)
        le.backward()
        w = want_grad.to(dtype).double()
        e = _log(name + ".dlogits(eager)", dtype, x.grad.double(), w, request.node.name)
        print(f"{request.node.name} {name} eager: loss rel {abs(float(le.detach()) - float(want_loss)) / float(want_loss):.3e}, dlogits norm-wise "
              f"{e:.3e}, max|err| / max|want| {float((x.grad.double() - w).abs().max() / w.abs().max()):.3e}")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_grid_stride_loop(cuda, dt, request):
    """More pixels than the capped workgroups cover in one pass.  At this pixel count the fp16 gradients of the plain loss are all
    subnormal, where one rounding flip is more than the allowance, so fp16 runs under the train step's loss scale."""
    dtype = DTYPES[dt]
    shape = _strided_shape(dtype, C=3 if dtype == torch.float16 else 2)
    N, C, H, W = shape
    up = 65536.0 if dtype == torch.float16 else 1.0
    for scale in (1.0, 8.0):
        logits, targets = make_case(cuda, shape, dtype, scale, seed=10)
        want_loss, want_grad = ref64(logits, targets, C, upstream=up)
        loss, grad = run_fused(logits, targets, C, upstream=lambda l: l.backward(torch.tensor(up, device=cuda)))
        name = f"seg_loss[grid-stride {N}x{C}x{H}x{W} scale {scale:g}]"
        check_loss(name, loss, want_loss, request.node.name)
        check_grad(name + ".dlogits", grad, want_grad, dtype, request.node.name)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("offset", (0, 1))
def test_channel_slice_views(cuda, dt, offset, request):
    """Logits as a channel slice of a wider tensor (batch and channel strides differ from the packed ones); with offset 1 the same
    view starts one element into its storage, which no 16-byte vector can reach."""
    dtype = DTYPES[dt]
    N, C, H, W = 3, 3, 16, 24
    for scale in (1.0, 8.0):
        packed, targets = make_case(cuda, (N, C, H, W), dtype, scale, seed=1)
        flat = torch.full((N * (C + 3) * H * W + offset,), float("nan"), dtype=dtype, device=cuda)
        wide = flat[offset:].view(N, C + 3, H, W)
        view = wide[:, 2:2 + C]
        view.copy_(packed)
        assert view.stride() == ((C + 3) * H * W, H * W, W, 1) and (view.data_ptr() % 16 == 0) == (offset == 0)
        want_loss, want_grad = ref64(packed, targets, C)
        loss, grad = run_fused(view, targets, C)
        name = f"seg_loss[slice offset {offset} scale {scale:g}]"
        check_loss(name, loss, want_loss, request.node.name)
        check_grad(name + ".dlogits", grad, want_grad, dtype, request.node.name)
        loss_p, grad_p = run_fused(packed, targets, C)
        assert torch.equal(loss, loss_p) and torch.equal(grad, grad_p)          # vector or element accesses: the same arithmetic
        assert bool(torch.isnan(wide[:, :2]).all()) and bool(torch.isnan(wide[:, 2 + C:]).all())


@pytest.mark.parametrize("case", ("35px", "vec", "ragged"))
def test_uint8_targets(cuda, case, request):
    for dt in ("fp32", "bf16"):
        dtype = DTYPES[dt]
        shape = GRID[case](dtype) if callable(GRID[case]) else GRID[case]
        C = shape[1]
        logits, t64 = make_case(cuda, shape, dtype, 4.0, seed=2)
        t8 = t64.to(torch.uint8)
        want_loss, want_grad = ref64(logits, t64, C)
        loss, grad = run_fused(logits, t8, C)
        check_loss(f"seg_loss[uint8 {case}]", loss, want_loss, request.node.name)
        check_grad(f"seg_loss[uint8 {case}].dlogits", grad, want_grad, dtype, request.node.name)
        loss64, grad64 = run_fused(logits, t64, C)
        assert torch.equal(loss, loss64) and torch.equal(grad, grad64)


@pytest.mark.parametrize("case", ("35px", "vec"))
def test_labels_outside_the_classes_belong_to_no_class(cuda, case, request):
    """uint8 255 (and int64 values that are no class) give an all-zero one-hot row: labels are compared, never used as an index."""
    shape = GRID[case]
    C = shape[1]
    for dtype in (torch.float32, torch.float16):
        logits, t64 = make_case(cuda, shape, dtype, 4.0, seed=3)
        g = torch.Generator().manual_seed(5)
        hole = (torch.rand(t64.shape, generator=g) < 0.2).to(cuda)
        t8 = t64.to(torch.uint8).masked_fill(hole, 255)
        want_loss, want_grad = ref64(logits, t8, C)
        loss, grad = run_fused(logits, t8, C)
        check_loss(f"seg_loss[255 {case}]", loss, want_loss, request.node.name)
        check_grad(f"seg_loss[255 {case}].dlogits", grad, want_grad, dtype, request.node.name)
        for other in (255, -1, C, 2 ** 32 + 1, -2 ** 40):
            loss_o, grad_o = run_fused(logits, t64.masked_fill(hole, other), C)
            assert torch.equal(loss_o, loss) and torch.equal(grad_o, grad), other


def test_upstream_gradient(cuda, request):
    shape = (3, 3, 16, 24)
    logits, targets = make_case(cuda, shape, torch.float32, 4.0, seed=4)
    want_loss, want_grad = ref64(logits, targets, 3, upstream=3.0)
    loss, grad = run_fused(logits, targets, 3, upstream=lambda l: (3 * l).backward())
    check_loss("seg_loss[3 * loss]", loss, want_loss, request.node.name)
    check_grad("seg_loss[3 * loss].dlogits", grad, want_grad, torch.float32, request.node.name)
    # fp16 logits under the train step's loss scale: multiplied in fp32 before the one rounding, so nothing is flushed
    for shape in ((3, 3, 16, 24), _ragged_shape(torch.float16, N=2)):
        logits, targets = make_case(cuda, shape, torch.float16, 4.0, seed=4)
        want_loss, want_grad = ref64(logits, targets, 3, upstream=65536.0)
        loss, grad = run_fused(logits, targets, 3,
                               upstream=lambda l: l.backward(torch.tensor(65536.0, device=cuda)))
        check_loss("seg_loss[65536]", loss, want_loss, request.node.name)
        check_grad("seg_loss[65536].dlogits", grad, want_grad, torch.float16, request.node.name)
        nz = want_grad.to(torch.float16) != 0
        assert bool((grad[nz] != 0).all())
        loss, grad = run_fused(logits, targets, 3, upstream=lambda l: (l * 65536.0).backward())
        check_grad("seg_loss[loss * 65536].dlogits", grad, want_grad, torch.float16, request.node.name)


def test_custom_alpha(cuda, request):
    logits, targets = make_case(cuda, (2, 3, 5, 7), torch.float32, 4.0, seed=6)
    alpha = (0.2, 0.5, 0.3)
    want_loss, want_grad = ref64(logits, targets, 3, alpha=alpha)
    for a in (alpha, torch.tensor(alpha, device=cuda)):
        loss, grad = run_fused(logits, targets, 3, alpha=a)
        check_loss("seg_loss[alpha]", loss, want_loss, request.node.name)
        check_grad("seg_loss[alpha].dlogits", grad, want_grad, torch.float32, request.node.name)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_repeatable_bits(cuda, dt):
    """No float atomics: a second call, a call on a side stream and a call under use_deterministic_algorithms give the same bits."""
    dtype = DTYPES[dt]
    shape = _ragged_shape(dtype, N=2)
    logits, targets = make_case(cuda, shape, dtype, 4.0, seed=7)
    loss0, grad0 = run_fused(logits, targets, 3)
    loss1, grad1 = run_fused(logits, targets, 3)
    assert torch.equal(loss0, loss1) and torch.equal(grad0, grad1)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        loss2, grad2 = run_fused(logits, targets, 3)
    side.synchronize()
    torch.cuda.current_stream(cuda).wait_stream(side)
    assert torch.equal(loss0, loss2) and torch.equal(grad0, grad2)
    torch.use_deterministic_algorithms(True)
    try:
        loss3, grad3 = run_fused(logits, targets, 3)
    finally:
        torch.use_deterministic_algorithms(False)
    assert torch.equal(loss0, loss3) and torch.equal(grad0, grad3)


def test_no_grad_saves_nothing(cuda):
    from vivim_amd import seg_loss
    logits, targets = make_case(cuda, (3, 3, 16, 24), torch.bfloat16, 4.0, seed=8)
    loss0, _ = run_fused(logits, targets, 3)
    x = logits.detach().requires_grad_(True)
    with torch.no_grad():
        loss1 = seg_loss.recall_focused_loss_fused(x, targets, 3)
    assert torch.equal(loss0, loss1) and not loss1.requires_grad and loss1.grad_fn is None
    loss2 = seg_loss.recall_focused_loss_fused(logits.detach(), targets, 3)          # logits that want no gradient
    assert torch.equal(loss0, loss2) and not loss2.requires_grad and loss2.grad_fn is None
    with pytest.raises(RuntimeError):
        loss1.backward()


def test_fallbacks_return_the_eager_loss(cuda):
    from vivim_amd import seg_loss
    from vivim_amd.train_step import recall_focused_loss
    logits, targets = make_case(cuda, (2, 3, 8, 8), torch.float32, 2.0, seed=9)
    assert not seg_loss.supported(logits, targets, 3, 3.0)
    assert torch.equal(seg_loss.recall_focused_loss_fused(logits, targets, 3, gamma=3.0), recall_focused_loss(logits, targets, 3, gamma=3.0))
    l9, t9 = make_case(cuda, (2, 9, 8, 8), torch.float32, 2.0, seed=9)
    assert not seg_loss.supported(l9, t9, 9, 2.0)
    assert torch.equal(seg_loss.recall_focused_loss_fused(l9, t9, 9), recall_focused_loss(l9, t9, 9))
    cl = logits.contiguous(memory_format=torch.channels_last)
    assert cl.stride(3) != 1 and not seg_loss.supported(cl, targets, 3, 2.0)
    a = cl.detach().requires_grad_(True)
    b = cl.detach().requires_grad_(True)
    la, lb = seg_loss.recall_focused_loss_fused(a, targets, 3), recall_focused_loss(b, targets, 3)
    assert torch.equal(la, lb)
    la.backward()
    lb.backward()
    assert torch.equal(a.grad, b.grad)


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
    clip, onehot = ts.synthetic_batch(2, 3, 24, 3, cuda, seed=11)
    out = {}
    for fused in (True, False):
        torch.manual_seed(12)
        model = _Stub(3).to(cuda)
        opt = ts.make_optimizer(model, lr=1e-2)
        del calls[:]
        losses = [float(ts.train_step(model, opt, clip, onehot, 3, amp_dtype=torch.float32, fused_loss=fused)) for _ in range(3)]
        names = [n for n in calls if n.startswith("vivim_seg_loss")]
        assert names == (["vivim_seg_loss_fwd", "vivim_seg_loss_bwd"] * 3 if fused else [])
        out[fused] = (losses, torch.cat([p.detach().flatten() for p in model.parameters()]))
    for a, b in zip(out[True][0], out[False][0]):
        assert abs(a - b) <= 1e-5 * abs(b), (out[True][0], out[False][0])
    e = rel_err(out[True][1], out[False][1])
    assert e < 1e-3, e
