"""fp64 references and error bounds for the channel-major LayerNorm family (csrc/layernorm.hip) and the depthwise convolution
(csrc/dwconv.hip), shared by tests/test_gpu_layernorm.py, test_gpu_add_norm.py and test_gpu_dwconv.py.  Everything here runs on the
CPU in float64 from the SAME rounded inputs the kernels get; gradients come from autograd.

LayerNorm, per token (the bounds of tests/test_gpu_layernorm_tm.py, applied to every row on its own):
    y        fp32 out: ||y - y64|| / ||y64|| <= 2e-6 + 4 * 2^-24 * |mean_r| / sqrt(var_r + eps); the second term is the rounding of the
             fp32 mean itself, which shifts the whole row.  16-bit out: one round-to-nearest of each element more, u_out (2^-8 bf16,
             2^-11 fp16: half a unit in the last of bf16's 8 and fp16's 11 significand bits).  A row of equal values (var 0) is
             compared absolutely: |y - bias| <= one rounding of bias to y's type.
    dx       fp32 1e-5, 16-bit u_io + 1e-5            dweight, dbias   1e-4 over the vector
    mean     |mean - mean64| <= 4 * 2^-24 * |mean64| + 2e-6 * sqrt(var_r + eps), rstd relative 2e-6: the two parts of y's bound (a mean
             off by d moves every xhat by d * rstd; a relative error of rstd is the same relative error of xhat).

Depthwise convolution, per element -- rigorous for fp32 accumulation in ANY order: the inputs are exact, every fma rounds once, and
a sum of n terms in any tree has error <= gamma_n * sum |terms| with gamma_n = n 2^-24 / (1 - n 2^-24) (Higham, Accuracy and
Stability of Numerical Algorithms, section 4.2):
    y, dx    |got - ref| <= gamma_28 * (sum_taps |w| |x| + |b|) + u_out * |ref| * (1 + 2^-20), u_out 2^-24 / 2^-11 / 2^-8
    dweight  gamma_(n + 64) * sum_tokens |dy| |x_shifted|, n = B D H W      dbias  gamma_(n + 64) * sum |dy|
(the + 64 covers the combine tree through LDS and atomics)."""
import os

import torch
import torch.nn.functional as F

import conftest

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
U_ROUND = {F32: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}           # unit roundoff 2^-p of a type with p significand bits
# (bf16 is 2^-8, not 2^-9: 1.198 rounds to 1.1953, off by 2.3e-3 = 0.98 * 2^-8 of the value; with 2^-9 the correctly rounded exact
# result would already miss a per-element bound, and test_fp64_bounds.py's ATen check shows it)
LN_SHAPES = [(2, 8, 40), (1, 64, 72), (2, 128, 40), (1, 320, 72), (2, 512, 40)]        # (B, C, L)
LN_FAMILIES = ("base", "shift", "ch0", "ch0_small", "mid", "ch0_shift", "const")


def name(dt):
    return str(dt).replace("torch.", "")


def gamma(n):
    return n * 2.0 ** -24 / (1.0 - n * 2.0 ** -24)


def log_ratio(what, dtype, shape, ratio):
    """The worst err / bound of a case, into the parity log."""
    try:
        os.makedirs(os.path.dirname(conftest._PARITY_LOG), exist_ok=True)
        with open(conftest._PARITY_LOG, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\t{what}\t{name(dtype)}\tshape={tuple(shape)}"
                    f"\tworst_err_over_bound={ratio:.3e}\n")
    except OSError:
        pass


# ---- LayerNorm

def ln_family(family, B, C, L, gen):
    """(B, L, C) fp32 rows of one input family (not yet rounded to the I/O type)."""
    r = torch.randn(B, L, C, generator=gen)
    if family == "base":
        return r * 1.7 + 0.4
    if family == "shift":
        return r + 30.0
    if family == "ch0":
        r[..., 0] = 40.0
        return r
    if family == "ch0_small":
        r *= 0.05
        r[..., 0] = 50.0
        return r
    if family == "mid":
        r *= 0.05
        r[..., C // 2] = 50.0
        return r
    if family == "ch0_shift":
        r += 30.0
        r[..., 0] = -40.0
        return r
    if family == "const":
        return torch.full((B, L, C), 2.5)
    raise ValueError(family)


def channel_major(x):
    """The same values as a (B, L, C) view of (B, C, L) memory: MambaLayer's view."""
    return x.transpose(1, 2).contiguous().transpose(1, 2)


def ln_reference(x, w, b, dy, eps):
    """F.layer_norm in fp64 of x as given (already rounded), gradients by autograd -> dict of fp64 tensors."""
    C = x.shape[-1]
    x64 = x.detach().double().contiguous().requires_grad_(True)
    w64 = w.detach().double().requires_grad_(True)
    b64 = None if b is None else b.detach().double().requires_grad_(True)
    y = F.layer_norm(x64, (C,), w64, b64, eps)
    y.backward(dy.detach().double())
    rows = x64.detach()
    return {"y": y.detach(), "dx": x64.grad, "dw": w64.grad, "db": None if b is None else b64.grad,
            "mean": rows.mean(dim=-1), "var": rows.var(dim=-1, unbiased=False)}


def ln_y_bound(x64, eps, out_dtype):
    """Per-row bound of ||y - y64|| / ||y64||, shape x64.shape[:-1]."""
    x64 = x64.detach().double()
    mean, var = x64.mean(dim=-1), x64.var(dim=-1, unbiased=False)
    tol = 2e-6 + 4 * 2.0 ** -24 * mean.abs() / (var + eps).sqrt()
    return tol + (0.0 if out_dtype == F32 else U_ROUND[out_dtype])


def ln_grad_bound(dtype):
    return 1e-5 + (0.0 if dtype == F32 else U_ROUND[dtype])


def row_ratio(got, want64, bound):
    """max over the rows of (||got - want|| / ||want||) / bound; `bound` a number or one value per row.  A row whose reference
    is all zero has to be zero."""
    C = want64.shape[-1]
    g, r = got.detach().double().cpu().reshape(-1, C), want64.reshape(-1, C)
    err = (g - r).norm(dim=1) / r.norm(dim=1).clamp_min(1e-30)
    b = bound.reshape(-1) if torch.is_tensor(bound) else torch.full_like(err, bound)
    return float((err / b).max())


def vec_ratio(got, want64, bound):
    return float((got.detach().double().cpu() - want64).norm() / want64.norm().clamp_min(1e-30)) / bound


def ln_ratios(got, ref, x64, eps, bias, ydt, xdt):
    """err / bound of every LayerNorm bound of this module for one call; `got`: dict with y, dx, dw, db (or None), mean, rstd (or None)
    as the kernel gave them, `ref`: ln_reference's, x64 the normalised rows.  y_const: rows of equal values, 0 when y is its bias
    to within one rounding of the bias to y's type, else inf."""
    x64 = x64.detach().double().cpu()
    var = x64.var(dim=-1, unbiased=False)
    flat = var == 0                                                     # rows of equal values: y = bias, compared absolutely
    r = {}
    y = got["y"].detach().double().cpu()
    if bool(flat.any()):
        b64 = torch.zeros(x64.shape[-1], dtype=torch.float64) if bias is None else bias.detach().double().cpu()
        allowed = (b64 - b64.float().to(ydt).double()).abs()            # one rounding of bias to y's type (0 for fp32)
        r["y_const"] = 0.0 if bool(((y - b64).abs() <= allowed)[flat].all()) else float("inf")
    if bool((~flat).any()):
        keep = ~flat
        r["y"] = row_ratio(y[keep], ref["y"][keep], ln_y_bound(x64[keep], eps, ydt))
    r["dx"] = row_ratio(got["dx"], ref["dx"], ln_grad_bound(xdt))
    r["dweight"] = vec_ratio(got["dw"], ref["dw"], 1e-4)
    if got.get("db") is not None:
        r["dbias"] = vec_ratio(got["db"], ref["db"], 1e-4)
    if got.get("mean") is not None:
        m, rs = got["mean"].detach().double().cpu(), got["rstd"].detach().double().cpu()
        std = (var + eps).sqrt()
        r["mean"] = float(((m - ref["mean"]).abs() / (4 * 2.0 ** -24 * ref["mean"].abs() + 2e-6 * std)).max())
        r["rstd"] = float(((rs * std - 1.0).abs() / 2e-6).max())
    return r


def ln_check(tag, got, ref, x64, eps, bias, ydt, xdt, worst):
    """Prints ln_ratios' figures, keeps the largest of each in `worst` and asserts that none is above 1."""
    r = ln_ratios(got, ref, x64, eps, bias, ydt, xdt)
    print(f"{tag}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items()) + " (err / bound)")
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, f"{tag}: err / bound above 1: {bad}"


# ---- depthwise convolution

def _conv(x, w, b, dims):
    """x (B, L, C) token-major -> the convolution on its (B, C, D, H, W) view, back to (B, L, C)."""
    B, L, C = x.shape
    D, H, W = dims
    xv = x.transpose(1, 2).reshape(B, C, D, H, W)
    if w.dim() == 4:
        y = F.conv2d(xv.reshape(B, C, H, W), w, b, padding=1, groups=C)
    else:
        y = F.conv3d(xv, w, b, padding=1, groups=C)
    return y.reshape(B, C, L).transpose(1, 2)


def dwconv_reference(x, w, b, dy, dims):
    """fp64 convolution and gradients of the given (rounded) inputs, and the per-element bounds of this module's docstring.
    -> (ref, bound): dicts with y, dx, dw and db (None without a bias); the bounds of y and dx for x's dtype as the output type."""
    u = U_ROUND[x.dtype]

    def run(xx, ww, bb, gg):
        xx, ww = xx.detach().double().requires_grad_(True), ww.detach().double().requires_grad_(True)
        bb = None if bb is None else bb.detach().double().requires_grad_(True)
        y = _conv(xx, ww, bb, dims)
        y.backward(gg.detach().double())
        return {"y": y.detach(), "dx": xx.grad, "dw": ww.grad, "db": None if bb is None else bb.grad}
    ref = run(x, w, b, dy)
    mag = run(x.detach().abs(), w.detach().abs(), None if b is None else b.detach().abs(), dy.detach().abs())
    n = x.shape[0] * x.shape[1]
    bound = {"y": gamma(28) * mag["y"] + u * ref["y"].abs() * (1 + 2.0 ** -20),
             "dx": gamma(28) * mag["dx"] + u * ref["dx"].abs() * (1 + 2.0 ** -20),
             "dw": gamma(n + 64) * mag["dw"], "db": None if b is None else gamma(n + 64) * mag["db"]}
    return ref, bound


def elem_ratio(got, want64, bound):
    """max over the elements of |got - want| / bound; an element whose bound is 0 (no term reaches it) has to be exact."""
    err = (got.detach().double().cpu() - want64).abs()
    assert bool((err[bound == 0] == 0).all())
    return float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
