"""csrc/token_layernorm.hip's residual add + LayerNorm / RMSNorm through vivim_amd.layernorm.add_layer_norm_tm / add_tm /
rms_norm_tm against fp64 on the CPU from the same (rounded) inputs.  Inputs, reference and bounds: tests/add_norm_tm_cases.py
(its docstring states the bounds); the reference norms THE res_new THE OP RETURNED."""
import os

import pytest
import torch

import add_norm_tm_cases as cases
import conftest
from add_norm_tm_cases import BF16, F16, F32, name

pytestmark = pytest.mark.gpu


def _log(what, dtype, shape, ratio):
    try:
        os.makedirs(os.path.dirname(conftest._PARITY_LOG), exist_ok=True)
        with open(conftest._PARITY_LOG, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\t{what}\t{name(dtype)}\tshape={tuple(shape)}"
                    f"\tmax_err_over_bound={ratio:.3e}\n")
    except OSError:
        pass


def _to_device(x, dev):
    """x on the device with the same sizes, strides and storage offset."""
    if x.is_contiguous() and x.storage_offset() == 0:
        return x.to(dev)
    n = x.untyped_storage().nbytes() // x.element_size()
    flat = torch.empty(n, dtype=x.dtype).set_(x.untyped_storage(), 0, (n,), (1,))
    return flat.to(dev).as_strided(x.shape, x.stride(), x.storage_offset())


def _run(inp, scale, bias, eps, rms, dev, use=("dy", "dres")):
    """One forward + backward of add_layer_norm_tm -> what cases.ratios reads."""
    from vivim_amd import layernorm as ln
    res = _to_device(inp["res"], dev).requires_grad_(True)
    branch = _to_device(inp["branch"], dev).requires_grad_(True)
    w = inp["w"].to(dev).requires_grad_(True)
    b = inp["b"].to(dev).requires_grad_(True) if bias else None
    sc = None if scale is None else scale.to(dev)
    assert ln.tm_add_supported(res, branch, w, b)
    res_new, y = ln.add_layer_norm_tm(res, branch, w, b, eps, scale=sc, rms=rms)
    assert res_new.dtype == res.dtype and res_new.shape == res.shape and res_new.is_contiguous()
    assert y.dtype == branch.dtype and y.shape == res.shape and y.is_contiguous()
    outs = [t for t, k in ((y, "dy"), (res_new, "dres")) if k in use]
    torch.autograd.backward(outs, [_to_device(inp[k], dev) for k in ("dy", "dres") if k in use])
    assert res.grad.dtype == res.dtype and branch.grad.dtype == branch.dtype and res.grad.shape == res.shape
    return {"res_new": res_new.detach(), "y": y.detach(), "dres_in": res.grad, "dbranch": branch.grad, "dw": w.grad,
            "db": None if b is None else b.grad}


def _check(tag, got, inp, scale, bias, eps, rms, btype, rtype, family, worst, use=("dy", "dres")):
    ref = cases.reference(got["res_new"].cpu(), inp["res"], inp["branch"], scale, inp["w"], inp["b"] if bias else None,
                          inp["dy"] if "dy" in use else None, inp["dres"] if "dres" in use else None, eps, rms)
    if "dy" not in use:
        got = dict(got, dw=None, db=None)
    r = cases.ratios(got, ref, scale, btype, rtype, family, eps, rms)
    print(tag + ": " + " ".join(f"{k}={v:.3f}" for k, v in r.items()) + "  (err / bound)")
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)
    assert all(v < 1.0 for v in r.values()), r


def _samples(shape):
    return shape[0]


@pytest.mark.parametrize("family", list(cases.FAMILIES))
@pytest.mark.parametrize("btype,rtype", cases.PAIRS, ids=lambda d: name(d))
@pytest.mark.parametrize("layout,shape", cases.SHAPES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_add_layer_norm_tm_against_fp64(layout, shape, btype, rtype, family, cuda):
    """LayerNorm and RMS, with and without bias, eps 1e-5 and 1e-6, scale None / ones / (1.25, 0, ...), on one input."""
    inp = cases.inputs(layout, shape, family, btype, rtype, seed=sum(shape) + 7 * len(shape))
    if layout.endswith("offset"):
        assert inp["branch" if layout.startswith("branch") else "res"].storage_offset() == 1
    worst = {}
    for rms, bias, eps, kind in cases.COMBOS:
        scale = cases.scale_of(kind, _samples(shape))
        got = _run(inp, scale, bias, eps, rms, cuda)
        _check(f"{layout} {shape} {name(btype)}/{name(rtype)} {family} rms={rms} bias={bias} eps={eps:g} scale={kind}", got, inp,
               scale, bias, eps, rms, btype, rtype, family, worst)
        assert (got["db"] is None) == (not bias)
    for k, v in worst.items():
        _log(f"add_layer_norm_tm {family} {k}", btype if k in ("y", "dbranch") else rtype, shape, v)


@pytest.mark.parametrize("family", list(cases.FAMILIES))
def test_more_than_1024_workgroups(family, cuda):
    """(4133, 512) fp32: the slot cap and the grid-stride loop of the backward."""
    layout, shape = cases.BIG
    inp = cases.inputs(layout, shape, family, F32, F32, seed=sum(shape) + 7 * len(shape))
    worst = {}
    for rms, bias, eps, kind in (cases.COMBOS[2], cases.COMBOS[4]):
        scale = cases.scale_of(kind, _samples(shape))
        got = _run(inp, scale, bias, eps, rms, cuda)
        _check(f"big {family} rms={rms}", got, inp, scale, bias, eps, rms, F32, F32, family, worst)
    for k, v in worst.items():
        _log(f"add_layer_norm_tm big {family} {k}", F32, shape, v)


@pytest.mark.parametrize("use", [("dy",), ("dres",), ("dy", "dres")], ids="+".join)
@pytest.mark.parametrize("btype,rtype", [(F32, F32), (BF16, F32), (F16, F16)], ids=lambda d: name(d))
def test_gradient_routing(btype, rtype, use, cuda):
    """dy alone (res_new unused), dres alone (y unused: dweight / dbias get no gradient), and both."""
    inp = cases.inputs("rows", (37, 64), "base", btype, rtype, seed=21)
    scale = cases.scale_of("drop", 37)
    for rms in (False, True):
        got = _run(inp, scale, True, 1e-5, rms, cuda, use=use)
        if "dy" not in use:
            assert got["dw"] is None and got["db"] is None
        _check(f"routing {use} rms={rms}", got, inp, scale, True, 1e-5, rms, btype, rtype, "base", {}, use=use)


@pytest.mark.parametrize("kind", [None, "ones", "drop"], ids=str)
@pytest.mark.parametrize("btype,rtype", cases.PAIRS, ids=lambda d: name(d))
@pytest.mark.parametrize("layout,shape", [("rows", (3, 5, 64)), ("rows", (7, 63)), ("branch_slice", (3, 5, 64)), ("res_offset", (7, 64))],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_add_tm_alone(layout, shape, btype, rtype, kind, cuda):
    """The forward within the res_new bound; dres_in is dres itself and dbranch = scale * dres to one rounding of its dtype."""
    from vivim_amd import layernorm as ln
    from fp64_bounds import U_ROUND
    inp = cases.inputs(layout, shape, "hard", btype, rtype, seed=31)
    scale = cases.scale_of(kind, shape[0])
    res = _to_device(inp["res"], cuda).requires_grad_(True)
    branch = _to_device(inp["branch"], cuda).requires_grad_(True)
    assert ln.tm_add_supported(res, branch)
    res_new = ln.add_tm(res, branch, scale=None if scale is None else scale.to(cuda))
    assert res_new.dtype == rtype and res_new.is_contiguous()
    res_new.backward(inp["dres"].to(cuda))
    ref = cases.reference(res_new.detach().cpu(), inp["res"], inp["branch"], scale, None, None, None, inp["dres"], 0.0, False)
    r = cases.sum_ratio(res_new, ref, rtype)
    print(f"add_tm {layout} {shape} {name(btype)}/{name(rtype)} scale={kind}: res_new={r:.3f} (err / bound)")
    assert r < 1.0
    assert torch.equal(res.grad.cpu(), inp["dres"])
    want = ref["dbranch"]
    err = (branch.grad.double().cpu() - want).abs()
    assert branch.grad.dtype == btype and bool((err <= (U_ROUND[btype] + 2.0 ** -24) * want.abs()).all())
    if scale is not None:
        assert bool((branch.grad.cpu()[scale == 0] == 0).all())
    _log("add_tm res_new", rtype, shape, r)


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=name)
def test_rms_norm_tm_and_the_no_residual_forward(dtype, cuda):
    from vivim_amd import layernorm as ln
    inp = cases.inputs("rows", (37, 64), "hard", dtype, dtype, seed=41)
    x64 = inp["branch"].double()
    # rms_norm_tm: y and dx of x itself
    x = inp["branch"].to(cuda).requires_grad_(True)
    w = inp["w"].to(cuda).requires_grad_(True)
    y = ln.rms_norm_tm(x, w, None, 1e-6)
    assert y.dtype == dtype and y.shape == x.shape
    y.backward(inp["dy"].to(cuda))
    ref = cases.reference(inp["branch"], None, inp["branch"], None, inp["w"], None, inp["dy"], None, 1e-6, True)
    got = {"res_new": inp["branch"], "y": y, "dbranch": x.grad, "dw": w.grad}
    r = cases.ratios(got, ref, None, dtype, dtype, "hard", 1e-6, True)
    print(f"rms_norm_tm {name(dtype)}: {r}")
    assert all(v < 1.0 for v in r.values()), r
    # no residual, the stream opened in fp32 (the first layer of a residual_in_fp32 stack): res_new is x itself, exactly
    for rms in (False, True):
        x = inp["branch"].to(cuda).requires_grad_(True)
        b = inp["b"].to(cuda).requires_grad_(True)
        res_new, y = ln.norm_tm_no_residual(x, w, b, 1e-5, rms, res_dtype=F32)
        assert res_new.dtype == F32 and torch.equal(res_new.double().cpu(), x64)
        torch.autograd.backward([y, res_new], [inp["dy"].to(cuda), inp["dres"].float().to(cuda)])
        ref = cases.reference(res_new.detach().cpu(), None, inp["branch"], None, inp["w"], inp["b"], inp["dy"], inp["dres"].float(),
                              1e-5, rms)
        got = {"res_new": res_new.detach(), "y": y, "dbranch": x.grad, "db": b.grad}
        r = cases.ratios(got, ref, None, dtype, F32, "hard", 1e-5, rms)
        print(f"no residual {name(dtype)} rms={rms}: {r}")
        assert all(v < 1.0 for v in r.values()), r


def _equal(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("layout,shape", [cases.BIG, ("rows", (67, 320)), ("res_offset", (7, 64)), ("rows", (3, 1000))],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
@pytest.mark.parametrize("btype,rtype", [(F32, F32), (BF16, F32), (BF16, BF16)], ids=lambda d: name(d))
def test_backward_twice_gives_equal_bits(layout, shape, btype, rtype, cuda):
    """dweight / dbias are slot sums in slot order, no atomics: two passes over one input agree bit for bit."""
    if (layout, shape) == cases.BIG and btype != F32:
        shape = (4133, 64)                               # the slot cap again, on a narrower row
    inp = cases.inputs(layout, shape, "base", btype, rtype, seed=3)
    scale = cases.scale_of("drop", shape[0])
    assert _equal(_run(inp, scale, True, 1e-5, False, cuda), _run(inp, scale, True, 1e-5, False, cuda))


def test_equal_bits_with_the_deterministic_flag_on_and_off(cuda):
    from vivim_amd import layernorm as ln
    inp = cases.inputs("rows", (3, 5, 64), "base", BF16, F32, seed=4)
    scale = cases.scale_of("drop", 3)
    plain = _run(inp, scale, True, 1e-5, False, cuda)
    torch.use_deterministic_algorithms(True)
    try:
        assert ln.tm_add_supported(inp["res"].to(cuda), inp["branch"].to(cuda), inp["w"].to(cuda), inp["b"].to(cuda))
        det = _run(inp, scale, True, 1e-5, False, cuda)
    finally:
        torch.use_deterministic_algorithms(False)
    assert _equal(plain, det)
    _check("deterministic", det, inp, scale, True, 1e-5, False, BF16, F32, "base", {})


@pytest.mark.parametrize("btype,rtype", [(F32, F32), (BF16, F32), (F16, F16)], ids=lambda d: name(d))
def test_no_grad_forward_has_the_same_bits_and_no_statistics(btype, rtype, cuda, monkeypatch):
    from vivim_amd import _lib
    from vivim_amd import layernorm as ln
    inp = cases.inputs("rows", (67, 320), "hard", btype, rtype, seed=5)
    scale = cases.scale_of("drop", 67)
    first = _run(inp, scale, True, 1e-5, False, cuda)
    seen = []
    real = _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda name, P, *a: (seen.append((name, P.mean, P.rstd)), real(name, P, *a))[1])
    args = (inp["w"].to(cuda), inp["b"].to(cuda), 1e-5)
    with torch.no_grad():
        a = ln.add_layer_norm_tm(inp["res"].to(cuda).requires_grad_(True), inp["branch"].to(cuda).requires_grad_(True), *args,
                                 scale=scale.to(cuda))
    b = ln.add_layer_norm_tm(inp["res"].to(cuda), inp["branch"].to(cuda), *args, scale=scale.to(cuda))   # nothing requires a gradient
    assert seen == [("vivim_token_add_norm_fwd", None, None)] * 2
    for res_new, y in (a, b):
        assert torch.equal(res_new, first["res_new"]) and torch.equal(y, first["y"]) and not y.requires_grad


def test_unsupported_dtype_pairs_raise(cuda):
    from vivim_amd import layernorm as ln
    w = torch.ones(64, device=cuda)
    for bt, rt in ((F32, BF16), (F32, F16), (F16, BF16), (BF16, F16), (torch.float64, torch.float64)):
        res, branch = torch.zeros(5, 64, device=cuda, dtype=rt), torch.zeros(5, 64, device=cuda, dtype=bt)
        assert not ln.tm_add_supported(res, branch, w)
        with pytest.raises(ValueError, match="not built"):
            ln.add_layer_norm_tm(res, branch, w, None)
        with pytest.raises(ValueError, match="not built"):
            ln.add_tm(res, branch)
    res, branch = torch.zeros(5, 64, device=cuda), torch.zeros(5, 64, device=cuda, dtype=BF16)
    with pytest.raises(ValueError, match="not built"):
        ln.add_layer_norm_tm(res, branch, w, None, out_dtype=F32)      # y is written in the branch's dtype
    with pytest.raises(ValueError, match="not built"):
        ln.rms_norm_tm(branch, w, out_dtype=F32)
    with pytest.raises(ValueError, match="scale"):
        ln.add_tm(res, branch, scale=torch.ones(4, device=cuda))
    assert not ln.tm_add_supported(res, branch, w.to(BF16))
    assert not ln.tm_add_supported(res[:, :32], branch)                                       # a shape mismatch
    assert not ln.tm_add_supported(torch.zeros(4, 6, 64, device=cuda)[:, :5], torch.zeros(4, 5, 64, device=cuda))   # two row strides
