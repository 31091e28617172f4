"""csrc/token_layernorm.hip through vivim_amd.layernorm.layer_norm_tm against torch.nn.functional.layer_norm in fp64 on the CPU,
from the same (rounded) inputs, the gradients from autograd.

Bounds (tests/test_gpu_layernorm.py's, here PER ROW for y and dx so that one wrong row cannot hide behind the others):
    y       fp32 < 2e-6, 16-bit < 4e-3          dx      fp32 < 1e-5, 16-bit < 4e-3          dweight, dbias < 1e-4 (over the vector)
and for an fp32 y of the hard family (randn + 30) 4 * 2^-24 * |mean_r| / std_r more: the fp32 mean's own rounding shifts the whole
row by that order.  A one-pass variance (E[x^2] - mean^2) misses the hard-family bound."""
import os

import pytest
import torch
import torch.nn.functional as F

import conftest

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
PAIRS = [(F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32), (F32, F16), (F32, BF16)]
# (layout, shape): plain rows; a 3-D tensor; a channel slice of wider rows (row stride 72); a view one element into its storage
SHAPES = [("rows", (37, 64)), ("rows", (130, 128)), ("rows", (67, 320)), ("rows", (19, 512)), ("rows", (5, 8)), ("rows", (9, 36)),
          ("rows", (3, 1000)), ("rows", (1, 64)), ("rows", (4133, 64)), ("rows", (2, 33, 64)), ("slice", (3, 5, 64)),
          ("offset", (7, 64))]
FAMILIES = {"base": (1.7, 0.4), "hard": (1.0, 30.0)}


def _name(dt):
    return str(dt).replace("torch.", "")


def _log(what, dtype, shape, err):
    try:
        os.makedirs(os.path.dirname(conftest._PARITY_LOG), exist_ok=True)
        with open(conftest._PARITY_LOG, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\t{what}\t{_name(dtype)}\tshape={tuple(shape)}"
                    f"\tmax_row_rel_err={err:.3e}\n")
    except OSError:
        pass


def _inputs(layout, shape, family, itype, otype, seed):
    """CPU tensors: x in its layout (a view where the layout says so), weight, bias, dy; already rounded to the I/O types."""
    gen = torch.Generator().manual_seed(seed)
    scale, shift = FAMILIES[family]
    C = shape[-1]
    if layout == "slice":
        x = torch.randn(*shape[:-1], C + 8, generator=gen).mul_(scale).add_(shift).to(itype)[..., :C]
    elif layout == "offset":
        n = 1
        for d in shape:
            n *= d
        x = torch.randn(n + 1, generator=gen).mul_(scale).add_(shift).to(itype)[1:].view(shape)
    else:
        x = torch.randn(*shape, generator=gen).mul_(scale).add_(shift).to(itype)
    w = torch.randn(C, generator=gen) * 0.5 + 1.0
    b = torch.randn(C, generator=gen) * 0.3
    dy = torch.randn(*shape, generator=gen).to(otype)
    return x, w, b, dy


def _to_device(x, dev):
    """x on the device with the same sizes, strides and storage offset."""
    if x.is_contiguous() and x.storage_offset() == 0:
        return x.to(dev)
    n = x.untyped_storage().nbytes() // x.element_size()
    flat = torch.empty(n, dtype=x.dtype).set_(x.untyped_storage(), 0, (n,), (1,))
    return flat.to(dev).as_strided(x.shape, x.stride(), x.storage_offset())


def _reference(x, w, b, dy, eps):
    x64 = x.double().contiguous().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    b64 = None if b is None else b.double().requires_grad_(True)
    y = F.layer_norm(x64, (x.shape[-1],), w64, b64, eps)
    y.backward(dy.double())
    return y.detach(), x64.grad, w64.grad, None if b is None else b64.grad, x64.detach()


def _row_err(got, want):
    """The largest per-row norm-wise relative error."""
    C = want.shape[-1]
    g, r = got.detach().double().cpu().reshape(-1, C), want.reshape(-1, C)
    return float(((g - r).norm(dim=1) / r.norm(dim=1).clamp_min(1e-30)).max())


def _vec_err(got, want):
    return float((got.detach().double().cpu() - want).norm() / want.norm().clamp_min(1e-30))


def _run(x, w, b, dy, eps, otype, dev):
    from vivim_amd import layernorm as ln
    xg = _to_device(x, dev).requires_grad_(True)
    wg = w.to(dev).requires_grad_(True)
    bg = None if b is None else b.to(dev).requires_grad_(True)
    assert ln.tm_supported(xg, wg, bg)
    y = ln.layer_norm_tm(xg, wg, bg, eps, out_dtype=otype)
    assert y.dtype == otype and y.shape == x.shape and y.is_contiguous()
    y.backward(_to_device(dy, dev))
    assert xg.grad.dtype == x.dtype and xg.grad.shape == x.shape
    return y, xg, wg, bg


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("itype,otype", PAIRS, ids=lambda d: _name(d))
@pytest.mark.parametrize("layout,shape", SHAPES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_layer_norm_tm_against_fp64(layout, shape, itype, otype, family, cuda):
    """With and without bias, eps 1e-5 and 1e-6, on one input."""
    from vivim_amd import layernorm as ln
    x, w, b, dy = _inputs(layout, shape, family, itype, otype, seed=sum(shape) + 7 * len(shape))
    if layout == "offset":
        assert x.storage_offset() == 1
    worst = {"y": 0.0, "dx": 0.0, "dweight": 0.0, "dbias": 0.0}
    for bias, eps in ((b, 1e-5), (None, 1e-5), (b, 1e-6), (None, 1e-6)):
        want_y, want_dx, want_dw, want_db, x64 = _reference(x, w, bias, dy, eps)
        y, xg, wg, bg = _run(x, w, bias, dy, eps, otype, cuda)
        C = shape[-1]
        y_tol = torch.full((x64.numel() // C,), 2e-6 if otype == F32 else 4e-3, dtype=torch.float64)
        if otype == F32 and family == "hard":
            rows = x64.reshape(-1, C)
            y_tol += 4 * 2.0 ** -24 * rows.mean(dim=1).abs() / rows.var(dim=1, unbiased=False).add(eps).sqrt()
        g, r = y.detach().double().cpu().reshape(-1, C), want_y.reshape(-1, C)
        y_err = (g - r).norm(dim=1) / r.norm(dim=1).clamp_min(1e-30)
        e = {"y": float(y_err.max()), "dx": _row_err(xg.grad, want_dx), "dweight": _vec_err(wg.grad, want_dw),
             "dbias": 0.0 if bias is None else _vec_err(bg.grad, want_db)}
        for k in e:
            worst[k] = max(worst[k], e[k])
        print(f"{layout} {shape} {_name(itype)}->{_name(otype)} {family} bias={bias is not None} eps={eps:g}: "
              + " ".join(f"{k}={v:.3e}" for k, v in e.items()) + f" (y bound {float(y_tol.min()):.3e}..{float(y_tol.max()):.3e})")
        assert bool((y_err < y_tol).all()), (float(y_err.max()), float(y_tol.min()))
        assert e["dx"] < (1e-5 if itype == F32 else 4e-3)
        assert e["dweight"] < 1e-4 and e["dbias"] < 1e-4
        assert (bg is None) == (bias is None)
    for k, v in worst.items():
        _log(f"layer_norm_tm {family} {k}", otype if k == "y" else itype, shape, v)
    assert not ln.supported(_to_device(x, cuda), w.to(cuda))                    # the channel-major family still refuses rows


@pytest.mark.parametrize("layout,shape", [("rows", (4133, 64)), ("rows", (67, 320)), ("offset", (7, 64)), ("rows", (3, 1000))],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
@pytest.mark.parametrize("itype,otype", [(F32, F32), (F32, BF16), (BF16, BF16)], ids=lambda d: _name(d))
def test_backward_twice_gives_equal_bits(layout, shape, itype, otype, cuda):
    """dweight / dbias are slot sums in slot order, no atomics: two backward passes of one input agree bit for bit."""
    x, w, b, dy = _inputs(layout, shape, "base", itype, otype, seed=3)
    first = _run(x, w, b, dy, 1e-5, otype, cuda)
    second = _run(x, w, b, dy, 1e-5, otype, cuda)
    assert torch.equal(first[0], second[0])
    for a, c in zip(first[1:], second[1:]):
        assert torch.equal(a.grad, c.grad)


def test_runs_and_matches_under_deterministic_algorithms(cuda):
    from vivim_amd import layernorm as ln
    x, w, b, dy = _inputs("rows", (2, 33, 64), "base", F32, F32, seed=4)
    plain = _run(x, w, b, dy, 1e-5, F32, cuda)
    torch.use_deterministic_algorithms(True)
    try:
        assert ln.tm_supported(plain[1].detach(), plain[2].detach(), plain[3].detach())
        det = _run(x, w, b, dy, 1e-5, F32, cuda)
    finally:
        torch.use_deterministic_algorithms(False)
    assert torch.equal(plain[0], det[0])
    for a, c in zip(plain[1:], det[1:]):
        assert torch.equal(a.grad, c.grad)
    want_y, want_dx, want_dw, want_db, _ = _reference(x, w, b, dy, 1e-5)
    assert _row_err(det[0], want_y) < 2e-6 and _row_err(det[1].grad, want_dx) < 1e-5
    assert _vec_err(det[2].grad, want_dw) < 1e-4 and _vec_err(det[3].grad, want_db) < 1e-4


@pytest.mark.parametrize("itype,otype", [(F32, F32), (F32, BF16), (F16, F32)], ids=lambda d: _name(d))
def test_no_grad_forward_has_the_same_bits_and_no_statistics(itype, otype, cuda, monkeypatch):
    from vivim_amd import _lib
    from vivim_amd import layernorm as ln
    x, w, b, dy = _inputs("rows", (67, 320), "hard", itype, otype, seed=5)
    y = _run(x, w, b, dy, 1e-5, otype, cuda)[0]
    seen = []
    real = _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda name, P, *a: (seen.append((name, P.mean, P.rstd)), real(name, P, *a))[1])
    with torch.no_grad():
        y0 = ln.layer_norm_tm(x.to(cuda).requires_grad_(True), w.to(cuda).requires_grad_(True), b.to(cuda), 1e-5, out_dtype=otype)
    y1 = ln.layer_norm_tm(x.to(cuda), w.to(cuda), b.to(cuda), 1e-5, out_dtype=otype)        # nothing requires a gradient
    assert seen == [("vivim_token_layernorm_fwd", None, None)] * 2
    assert torch.equal(y0, y.detach()) and torch.equal(y1, y.detach()) and not y0.requires_grad


def test_output_dtype_follows_aten_and_bad_pairs_are_refused(cuda):
    from vivim_amd import layernorm as ln
    x, w = torch.randn(5, 64, device=cuda, dtype=BF16), torch.ones(64, device=cuda)
    assert ln.layer_norm_tm(x, w, None).dtype == BF16
    with torch.autocast("cuda", dtype=BF16):
        assert ln.layer_norm_tm(x, w, None).dtype == F.layer_norm(x, (64,), w, None).dtype == F32
    with pytest.raises(ValueError, match="not built"):
        ln.layer_norm_tm(x, w, None, out_dtype=F16)
    assert not ln.tm_supported(x, w.to(BF16), None) and not ln.tm_supported(x.cpu(), w, None)
    assert not ln.tm_supported(torch.randn(5, 128, device=cuda)[:, ::2], w, None)
    assert not ln.tm_supported(torch.randn(4, 6, 64, device=cuda)[:, :5], w, None)          # two row strides
    assert ln.tm_supported(torch.randn(4, 6, 72, device=cuda)[..., :64], w, None)
