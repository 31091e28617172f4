"""tests/fp64_bounds.py checked against itself on the CPU: the bounds it states hold for ANY fp32 implementation of the two
operations, so ATen's own fp32 kernels must meet them -- the convolution by the gamma_n theorem, the LayerNorm by measurement
(ATen's fp32 layer_norm stays below 0.4 of the per-token bound on every input family at every channel count of the GPU tests)."""
import pytest
import torch
import torch.nn.functional as F

import fp64_bounds as fb
from fp64_bounds import BF16, F16, F32

DW_SHAPES = [(2, 1, 1, 1, 8), (2, 3, 2, 3, 8), (1, 2, 5, 7, 24), (2, 2, 3, 9, 136)]     # (B, D, H, W, C)


def test_gamma():
    assert fb.gamma(1) == pytest.approx(2.0 ** -24, rel=1e-6) and fb.gamma(28) > 28 * 2.0 ** -24
    assert fb.gamma(28) < 28 * 2.0 ** -24 * (1 + 1e-5)


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=fb.name)
@pytest.mark.parametrize("B,D,H,W,C,k3,has_bias", [s + (True, True) for s in DW_SHAPES] + [s + (False, False) for s in DW_SHAPES if s[1] == 1])
def test_aten_fp32_conv_meets_the_dwconv_bound(B, D, H, W, C, k3, has_bias, dtype):
    gen = torch.Generator().manual_seed(B + D + H + W + C)
    L = D * H * W
    x = torch.randn(B, L, C, generator=gen).to(dtype)
    w = torch.randn(*((C, 1, 3, 3, 3) if k3 else (C, 1, 3, 3)), generator=gen) * 0.3
    b = torch.randn(C, generator=gen) if has_bias else None
    dy = torch.randn(B, L, C, generator=gen).to(dtype)
    ref, bound = fb.dwconv_reference(x, w, b, dy, (D, H, W))
    x32, w32 = x.float().requires_grad_(True), w.clone().requires_grad_(True)
    b32 = None if b is None else b.clone().requires_grad_(True)
    y = fb._conv(x32, w32, b32, (D, H, W))
    y.backward(dy.float())
    assert fb.elem_ratio(y.to(dtype), ref["y"], bound["y"]) <= 1.0
    assert fb.elem_ratio(x32.grad.to(dtype), ref["dx"], bound["dx"]) <= 1.0
    assert fb.elem_ratio(w32.grad, ref["dw"], bound["dw"]) <= 1.0
    if has_bias:
        assert fb.elem_ratio(b32.grad, ref["db"], bound["db"]) <= 1.0
    # and the bound bites: one tap skipped at one border position is far outside it
    if W > 1:
        tap = w[:, 0, 1, 1, 0] if k3 else w[:, 0, 1, 0]                   # the centre row's tap that reads w - 1
        broken = y.detach().reshape(B, D, H, W, C).clone()
        broken[:, :, :, W - 1] -= x.float().reshape(B, D, H, W, C)[:, :, :, W - 2] * tap
        assert fb.elem_ratio(broken.reshape(B, L, C).to(dtype), ref["y"], bound["y"]) > 1.0


@pytest.mark.parametrize("family", fb.LN_FAMILIES)
@pytest.mark.parametrize("B,C,L", fb.LN_SHAPES)
def test_aten_fp32_layer_norm_is_inside_the_per_token_bound(B, C, L, family):
    gen = torch.Generator().manual_seed(C + L)
    x = fb.ln_family(family, B, C, L, gen)
    w, b = torch.randn(C, generator=gen) * 0.5 + 1.0, torch.randn(C, generator=gen) * 0.3
    dy = torch.randn(B, L, C, generator=gen)
    ref = fb.ln_reference(x, w, b, dy, 1e-5)
    x32, w32, b32 = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.layer_norm(x32, (C,), w32, b32, 1e-5)
    y.backward(dy)
    worst = {}
    fb.ln_check(f"ATen fp32 {family} {(B, C, L)}", {"y": y, "dx": x32.grad, "dw": w32.grad, "db": b32.grad}, ref, x, 1e-5, b, F32, F32,
                worst)
    assert worst.get("y", 0.0) <= 0.5                 # the reference implementation alone is well inside the bound


def test_one_pass_variance_is_outside_the_bound():
    """The defect the per-token bound exists for: E[d^2] - E[d]^2 around channel 0 in fp32 with an outlier in channel 0."""
    gen = torch.Generator().manual_seed(1)
    C = 512
    x = fb.ln_family("ch0", 2, C, 40, gen)
    w, b = torch.ones(C), torch.zeros(C)
    d = x - x[..., :1]
    m = d.sum(-1) / C
    rstd = torch.rsqrt((d * d).sum(-1) / C - m * m + 1e-5)
    y = (x - (x[..., 0] + m)[..., None]) * rstd[..., None]
    ref = fb.ln_reference(x, w, b, torch.zeros_like(x), 1e-5)
    assert fb.row_ratio(y, ref["y"], fb.ln_y_bound(x, 1e-5, F32)) > 1.0
