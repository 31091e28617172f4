"""csrc/layernorm.hip (the LayerNorms around the Mamba call, modeling/vivim.py:155-156) through the C ABI
(vivim_amd/layernorm.py).  Per TOKEN against F.layer_norm in fp64 on the CPU (tests/fp64_bounds.py, the bounds of
test_gpu_layernorm_tm.py): y fp32 < 2e-6 + 4 * 2^-24 * |mean_r| / std_r, 16-bit that plus one rounding (2^-8 bf16, 2^-11 fp16);
dx fp32 < 1e-5, 16-bit one rounding more; dweight, dbias < 1e-4 over the vector; on benign, shifted, outlier-channel and constant rows.
And, at the bench's sizes, one Frobenius norm against fp32 F.layer_norm -- the operator the reference uses there."""
import pytest
import torch
import torch.nn.functional as F

import fp64_bounds as fb
from conftest import rel_err

pytestmark = pytest.mark.gpu


def _cm(B, C, L, dtype, dev, gen):
    """(B, L, C) view of (B, C, L) memory, as MambaLayer builds it."""
    return torch.randn(B, C, L, generator=gen).mul_(1.7).add_(0.4).to(dtype).to(dev).transpose(1, 2)


@pytest.mark.parametrize("B,C,L", [(3, 64, 20480), (2, 128, 5120), (2, 320, 1280), (3, 512, 320), (1, 96, 40), (2, 8, 8)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("tile", [None, "8", "16", "32"])
def test_layer_norm_channel_major(B, C, L, dtype, autocast, tile, cuda, monkeypatch):
    """Every tile length of the kernels (VIVIM_LN_TT: tokens per wave; None = the automatic choice; a length that does not fit
    the shape -- LDS, or 16 tokens of a 16-bit row of 8-element vectors -- falls back to the next one that does)."""
    from vivim_amd import layernorm as ln
    if tile is None:
        monkeypatch.delenv("VIVIM_LN_TT", raising=False)
    else:
        monkeypatch.setenv("VIVIM_LN_TT", tile)
    gen = torch.Generator().manual_seed(C + L)
    x = _cm(B, C, L, dtype, cuda, gen).requires_grad_(True)
    w = (torch.randn(C, generator=gen) * 0.5 + 1.0).to(cuda).requires_grad_(True)
    b = (torch.randn(C, generator=gen) * 0.3).to(cuda).requires_grad_(True)
    assert ln.supported(x, w)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = ln.layer_norm_cm(x, w, b, 1e-5)
        # ATen: f32 under autocast (layer_norm is on its fp32 list), the input's dtype otherwise (it then wants the weights in
        # that dtype too; the fused op keeps them f32 either way)
        want_dtype = F.layer_norm(x.detach(), (C,), w.detach(), b.detach(), 1e-5).dtype if autocast else dtype
    assert y.dtype == want_dtype and y.shape == (B, L, C) and y.is_contiguous()
    g = torch.randn(B, L, C, generator=gen).to(y.dtype).to(cuda)
    y.backward(g)
    # reference: fp32 layer_norm of the same (rounded) inputs, gradient by autograd
    x32 = x.detach().float().requires_grad_(True)
    w32, b32 = w.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    r = F.layer_norm(x32, (C,), w32, b32, 1e-5)
    r.backward(g.float())
    lo = y.dtype != torch.float32
    assert rel_err(y.float(), r.to(y.dtype).float()) < (4e-3 if lo else 2e-6)
    assert x.grad.shape == x.shape and x.grad.stride() == x.stride()          # dx in x's own (channel-major) layout
    gx_tol = 4e-3 if dtype != torch.float32 else 1e-5
    assert rel_err(x.grad.float(), x32.grad.to(dtype).float()) < gx_tol
    assert rel_err(w.grad, w32.grad) < 1e-4 and rel_err(b.grad, b32.grad) < 1e-4


_REF = {}


@pytest.mark.parametrize("B,C,L", fb.LN_SHAPES)
@pytest.mark.parametrize("itype,otype", [(fb.F32, fb.F32), (fb.BF16, fb.BF16), (fb.F16, fb.F16), (fb.BF16, fb.F32), (fb.F16, fb.F32)],
                         ids=fb.name)
@pytest.mark.parametrize("tile", [None, "8", "16", "32"])
def test_layer_norm_cm_per_token_against_fp64(B, C, L, itype, otype, tile, cuda, monkeypatch):
    """Every input family of fp64_bounds.LN_FAMILIES, with and without bias, every tile length (the chain of the per-token sums is
    C * TT / 64 long): y, dx, dweight, dbias and the saved mean / rstd against fp64, per token.  An fp32 y from 16-bit rows is the
    autocast case.  Before the statistics took their second sweep over the tile, the fp32-output rows with the outlier in channel 0
    missed y's bound at every C >= 64 (the figures are in profiles/r09_layernorm_stats.txt)."""
    from vivim_amd import layernorm as ln
    if tile is None:
        monkeypatch.delenv("VIVIM_LN_TT", raising=False)
    else:
        monkeypatch.setenv("VIVIM_LN_TT", tile)
    for family in fb.LN_FAMILIES:
        worst = {}
        for has_bias in (True, False):
            key = (B, C, L, itype, otype, family, has_bias)
            if key not in _REF:
                gen = torch.Generator().manual_seed(C + L)
                x = fb.channel_major(fb.ln_family(family, B, C, L, gen).to(itype))
                w = torch.randn(C, generator=gen) * 0.5 + 1.0
                b = torch.randn(C, generator=gen) * 0.3 if has_bias else None
                dy = torch.randn(B, L, C, generator=gen).to(otype)
                _REF[key] = (x, w, b, dy, fb.ln_reference(x, w, b, dy, 1e-5))
            x, w, b, dy, ref = _REF[key]
            xg = x.transpose(1, 2).to(cuda).transpose(1, 2).requires_grad_(True)
            wg = w.to(cuda).requires_grad_(True)
            bg = None if b is None else b.to(cuda).requires_grad_(True)
            assert ln.supported(xg, wg) and xg.stride() == (C * L, 1, L)
            y = ln.layer_norm_cm(xg, wg, bg, 1e-5, out_dtype=otype)
            assert y.dtype == otype and y.shape == (B, L, C) and y.is_contiguous()
            stats = y.grad_fn.saved_tensors[2]                                  # (2, B, L): mean, rstd as the backward will read them
            y.backward(dy.to(cuda))
            assert xg.grad.dtype == itype and xg.grad.stride() == xg.stride()
            got = {"y": y, "dx": xg.grad, "dw": wg.grad, "db": None if bg is None else bg.grad, "mean": stats[0], "rstd": stats[1]}
            fb.ln_check(f"{family} {(B, C, L)} {fb.name(itype)}->{fb.name(otype)} TT={tile} bias={has_bias}", got, ref, x, 1e-5, b,
                        otype, itype, worst)
        for k, v in worst.items():
            fb.log_ratio(f"layer_norm_cm TT={tile} {family} {k}", otype if k == "y" else itype, (B, C, L), v)


def test_layer_norm_no_bias_and_unsupported_layouts(cuda):
    from vivim_amd import layernorm as ln
    gen = torch.Generator().manual_seed(2)
    x = _cm(2, 64, 256, torch.float32, cuda, gen)
    w = torch.ones(64, device=cuda)
    y = ln.layer_norm_cm(x, w, None, 1e-6)
    assert rel_err(y, F.layer_norm(x, (64,), w, None, 1e-6)) < 2e-6
    assert not ln.supported(x.contiguous(), w)                                # token-major rows: ATen's kernel is the right one
    assert not ln.supported(_cm(1, 1024, 64, torch.float32, cuda, gen), torch.ones(1024, device=cuda))   # > 512 channels
    assert not ln.supported(_cm(1, 64, 36, torch.bfloat16, cuda, gen), w)     # 36 tokens: not whole 16-byte pieces


def test_mamba_layer_uses_the_fused_norm(cuda, monkeypatch):
    """MambaLayer with and without the fused norm: same output and parameter gradients (the norm's nn.LayerNorm parameters and
    state-dict keys are untouched)."""
    from modeling.vivim import MambaLayer
    from vivim_amd import layernorm as ln
    torch.manual_seed(5)
    layer = MambaLayer(64).to(cuda)
    x = torch.randn(2, 64, 2, 32, 32, device=cuda)          # 4 096 tokens: above layernorm.worthwhile's threshold
    calls = []
    real = ln.layer_norm_cm
    monkeypatch.setattr(ln, "layer_norm_cm", lambda *a: (calls.append(1), real(*a))[1])

    def run():
        for p in layer.parameters():
            p.grad = None
        y = layer(x)
        y.square().mean().backward()
        return y.detach(), {n: p.grad.clone() for n, p in layer.named_parameters()}
    y1, g1 = run()
    assert len(calls) == 2                                   # norm1 and norm2 both took the kernel
    monkeypatch.setenv("VIVIM_NO_FUSED_LAYERNORM", "1")
    y2, g2 = run()
    assert len(calls) == 2
    assert not ln.worthwhile(torch.empty(3, 320, 512, device=cuda)) and ln.worthwhile(torch.empty(3, 5120, 128, device=cuda))
    assert rel_err(y1, y2) < 1e-5
    for n in g1:
        assert rel_err(g1[n], g2[n]) < 2e-4, n
    assert {"norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"} <= set(g1)
