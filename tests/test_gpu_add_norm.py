"""csrc/layernorm.hip with the add: the residual add fused with the LayerNorm that follows it (vivim_amd/layernorm.py: add_layer_norm_cm,
add_cm; MambaLayer(fused_add_norm=True)) against an fp64 reference built from the same rounded inputs.  Per TOKEN (tests/fp64_bounds.py,
the bounds of test_gpu_layernorm_tm.py): y fp32 < 2e-6 + 4 * 2^-24 * |mean_r| / std_r, 16-bit that plus one rounding (2^-8 bf16, 2^-11
fp16); dx, dbranch fp32 < 1e-5, 16-bit one rounding more; dweight, dbias < 1e-4 over the vector; x_new within one rounding of the
rounded reference; on benign, shifted, outlier-channel and constant rows of x_new.  And one Frobenius norm per tensor at larger sizes."""
import pytest
import torch
import torch.nn.functional as F

import fp64_bounds as fb
from conftest import rel_err

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
PAIRS = [(F32, F32), (BF16, BF16), (F16, F16), (F32, BF16), (F32, F16)]             # (x, branch)
SHAPES = [(2, 8, 8), (1, 96, 40), (2, 320, 1280), (3, 512, 320), (2, 64, 1000)]    # (B, C, L)


def _tol_y(dtype):
    return 2e-6 if dtype == F32 else 4e-3


def _tol_g(dtype):
    return 1e-5 if dtype == F32 else 4e-3


def _inputs(B, C, L, xdt, bdt, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, L, generator=gen).mul_(1.7).add_(0.4).to(xdt).to(dev).transpose(1, 2)     # MambaLayer's view
    br = torch.randn(B, L, C, generator=gen).mul_(0.8).to(bdt).to(dev)
    w = (torch.randn(C, generator=gen) * 0.5 + 1.0).to(dev)
    b = (torch.randn(C, generator=gen) * 0.3).to(dev)
    scale = None
    if B > 1:                                                                      # DropPath at keep 0.75, one sample dropped
        scale = torch.full((B,), 1 / 0.75)
        scale[B // 2] = 0.0
        scale = scale.to(dev)
    gres = torch.randn(B, C, L, generator=gen).to(xdt).to(dev).transpose(1, 2)      # arrives channel-major, like x
    gy = torch.randn(B, L, C, generator=gen)
    return x, br, w, b, scale, gres, gy.to(dev)


_REF = {}


def _reference(key, x, br, w, b, scale, gres, gy, norm=True):
    """fp64, from the same rounded inputs: x64 + s * b64, rounded to x's dtype (straight-through for the gradient), then
    F.layer_norm in fp64; gradients by autograd.  Computed once per (shape, dtypes, dtype of y) and shared.

    The rounding goes through fp32, spelled out: that is the op's contract (accumulated in fp32, rounded once from there), what
    a 16-bit torch add does and how torch converts fp64 to a 16-bit type.  Rounding the exact sum straight to float16 (what a
    fused fma with an f16 result does) is a different function: with s = 4 / 3 it differs by one ulp in 3.4 % of the elements
    (x + 4 v / 3 sits on a 16-bit midpoint whenever 3 divides v's mantissa; only the low bits of fp32(4 / 3) break the tie),
    which moves dweight by more than its 1e-4."""
    if key in _REF:
        return _REF[key]
    x64, b64 = x.detach().double().requires_grad_(True), br.detach().double().requires_grad_(True)
    s = scale.double()[:, None, None] if scale is not None else 1.0
    exact = x64 + s * b64
    xn = exact + (exact.detach().float().to(x.dtype).double() - exact.detach())
    loss = (xn * gres.double()).sum()
    out = {"x_new": xn.detach()}
    if norm:
        w64, bias64 = w.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True)
        y = F.layer_norm(xn, (x.shape[2],), w64, bias64, 1e-5)
        loss = loss + (y * gy.double()).sum()
        out["y"] = y.detach()
    loss.backward()
    out.update(dx=x64.grad, dbranch=b64.grad)
    if norm:
        out.update(dw=w64.grad, db=bias64.grad)
    _REF[key] = out
    return out


def _check(name, got, want64, dtype, tol):
    e = rel_err(got.float(), want64.to(dtype).float())
    print(f"{name}: rel_err {e:.3e} (bound {tol:.0e})")
    assert e < tol, f"{name}: {e:.3e} >= {tol:.0e}"


def _set_tile(monkeypatch, tile):
    if tile is None:
        monkeypatch.delenv("VIVIM_LN_TT", raising=False)
    else:
        monkeypatch.setenv("VIVIM_LN_TT", tile)


@pytest.mark.parametrize("B,C,L", SHAPES)
@pytest.mark.parametrize("xdt,bdt", PAIRS)
@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("tile", [None, "8", "16", "32"])
def test_add_layer_norm_against_fp64(B, C, L, xdt, bdt, autocast, tile, cuda, monkeypatch):
    from vivim_amd import layernorm as ln
    _set_tile(monkeypatch, tile)
    x, br, w, b, scale, gres, gy = _inputs(B, C, L, xdt, bdt, cuda, C + L)
    x.requires_grad_(True), br.requires_grad_(True), w.requires_grad_(True), b.requires_grad_(True)
    assert ln.add_norm_supported(x, br, w)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        x_new, y = ln.add_layer_norm_cm(x, br, w, b, 1e-5, scale)
    ydt = F32 if autocast else xdt
    assert y.dtype == ydt and y.shape == (B, L, C) and y.is_contiguous()
    assert x_new.dtype == xdt and x_new.shape == x.shape and x_new.stride() == x.stride()
    gy = gy.to(ydt)
    torch.autograd.backward([x_new, y], [gres, gy])
    ref = _reference((B, C, L, xdt, bdt, ydt), x, br, w, b, scale, gres, gy)
    _check("x_new", x_new, ref["x_new"], xdt, _tol_y(xdt))
    _check("y", y, ref["y"], ydt, _tol_y(ydt))
    assert x.grad.shape == x.shape and x.grad.stride() == x.stride()               # dx in x's own (channel-major) layout
    assert br.grad.dtype == bdt and br.grad.shape == br.shape
    _check("dx", x.grad, ref["dx"], xdt, _tol_g(xdt))
    _check("dbranch", br.grad, ref["dbranch"], bdt, _tol_g(bdt))
    _check("dweight", w.grad, ref["dw"], F32, 1e-4)
    _check("dbias", b.grad, ref["db"], F32, 1e-4)
    if scale is not None:                                                          # the dropped sample, exactly
        z = B // 2
        assert torch.equal(x_new[z], x[z]) and not bool(br.grad[z].any())


_FAM = {}


def _family_inputs(B, C, L, xdt, bdt, ydt, family, scaled):
    """CPU tensors: x holds the family's rows, the branch is small (zero for the constant rows) so that x_new = x + s * branch
    keeps the pattern; the reference and the bounds see x_new as the op's contract rounds it."""
    key = (B, C, L, xdt, bdt, ydt, family, scaled)
    if key not in _FAM:
        gen = torch.Generator().manual_seed(C + L)
        x = fb.channel_major(fb.ln_family(family, B, C, L, gen).to(xdt))
        br = (torch.randn(B, L, C, generator=gen) * (0.0 if family == "const" else 0.01)).to(bdt)
        w, b = torch.randn(C, generator=gen) * 0.5 + 1.0, torch.randn(C, generator=gen) * 0.3
        scale = None
        if scaled:                                                                 # DropPath at keep 0.75; with B > 1 one sample dropped
            scale = torch.full((B,), 1 / 0.75)
            if B > 1:
                scale[B // 2] = 0.0
        gres = fb.channel_major(torch.randn(B, L, C, generator=gen).to(xdt))
        gy = torch.randn(B, L, C, generator=gen).to(ydt)
        ref = _reference(key, x, br, w, b, scale, gres, gy)
        rows = ref["x_new"]
        ref = dict(ref, mean=rows.mean(dim=-1), var=rows.var(dim=-1, unbiased=False))
        _FAM[key] = (x, br, w, b, scale, gres, gy, ref)
    return _FAM[key]


@pytest.mark.parametrize("B,C,L", fb.LN_SHAPES)
@pytest.mark.parametrize("xdt,bdt", PAIRS, ids=fb.name)
@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("tile", [None, "8", "16", "32"])
def test_add_layer_norm_per_token_against_fp64(B, C, L, xdt, bdt, autocast, tile, cuda, monkeypatch):
    """Every input family of fp64_bounds.LN_FAMILIES as rows of x_new, with and without the per-sample scale, every tile length:
    x_new, y, dx, dbranch, dweight, dbias and the saved mean / rstd against fp64, per token.  The add mode shares the plain mode's
    statistics: with the one-sweep variance its fp32-output rows with the outlier in channel 0 missed y's bound in the same way."""
    from vivim_amd import layernorm as ln
    _set_tile(monkeypatch, tile)
    ydt = F32 if autocast else xdt
    to_cm = lambda t: t.transpose(1, 2).to(cuda).transpose(1, 2)                   # keeps the channel-major strides
    for family in fb.LN_FAMILIES:
        worst = {}
        for scaled in (True, False):
            x, br, w, b, scale, gres, gy, ref = _family_inputs(B, C, L, xdt, bdt, ydt, family, scaled)
            xg, bg = to_cm(x).requires_grad_(True), br.to(cuda).requires_grad_(True)
            wg, biasg = w.to(cuda).requires_grad_(True), b.to(cuda).requires_grad_(True)
            sg = None if scale is None else scale.to(cuda)
            assert ln.add_norm_supported(xg, bg, wg)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                x_new, y = ln.add_layer_norm_cm(xg, bg, wg, biasg, 1e-5, sg)
            assert y.dtype == ydt and y.is_contiguous() and x_new.dtype == xdt and x_new.stride() == xg.stride()
            stats = y.grad_fn.saved_tensors[2]                                     # (2, B, L): mean, rstd as the backward will read them
            torch.autograd.backward([x_new, y], [to_cm(gres), gy.to(cuda)])
            tag = f"{family} {(B, C, L)} {fb.name(xdt)}+{fb.name(bdt)}->{fb.name(ydt)} TT={tile} scale={scaled}"
            got = {"y": y, "dx": xg.grad, "dw": wg.grad, "db": biasg.grad, "mean": stats[0], "rstd": stats[1]}
            extra = {"x_new": fb.row_ratio(x_new, ref["x_new"], 2e-6 if xdt == F32 else fb.U_ROUND[xdt]),
                     "dbranch": fb.row_ratio(bg.grad, ref["dbranch"], fb.ln_grad_bound(bdt))}
            print(f"{tag}: x_new={extra['x_new']:.3f} dbranch={extra['dbranch']:.3f} (err / bound)")
            for k, v in extra.items():
                worst[k] = max(worst.get(k, 0.0), v)
            fb.ln_check(tag, got, ref, ref["x_new"], 1e-5, b, ydt, xdt, worst)
            assert extra["x_new"] <= 1.0 and extra["dbranch"] <= 1.0, (tag, extra)
            if scaled and B > 1:                                                   # the dropped sample, exactly
                z = B // 2
                assert torch.equal(x_new[z], xg[z]) and not bool(bg.grad[z].any())
        for k, v in worst.items():
            fb.log_ratio(f"add_layer_norm_cm TT={tile} {family} {k}", ydt if k == "y" else bdt if k == "dbranch" else xdt, (B, C, L), v)


@pytest.mark.parametrize("xdt,bdt", PAIRS)
@pytest.mark.parametrize("norm", [True, False])
def test_unscaled_sum_is_torchs_add_bit_for_bit(xdt, bdt, norm, cuda):
    """scale None: one correctly rounded add has one result."""
    from vivim_amd import layernorm as ln
    for B, C, L in ((1, 96, 40), (2, 64, 1000)):
        x, br, w, b, _, _, _ = _inputs(B, C, L, xdt, bdt, cuda, 7)
        x_new = ln.add_layer_norm_cm(x, br, w, b, 1e-5)[0] if norm else ln.add_cm(x, br)
        want = x + br
        assert want.dtype == x_new.dtype and torch.equal(x_new, want)


@pytest.mark.parametrize("B,C,L", SHAPES)
@pytest.mark.parametrize("xdt,bdt", PAIRS)
@pytest.mark.parametrize("tile", [None, "8", "32"])
def test_add_cm_against_fp64(B, C, L, xdt, bdt, tile, cuda, monkeypatch):
    from vivim_amd import layernorm as ln
    _set_tile(monkeypatch, tile)
    x, br, w, b, scale, gres, gy = _inputs(B, C, L, xdt, bdt, cuda, C + L)
    x.requires_grad_(True), br.requires_grad_(True)
    assert ln.add_norm_supported(x, br, None)
    x_new = ln.add_cm(x, br, scale)
    assert x_new.dtype == xdt and x_new.stride() == x.stride()
    x_new.backward(gres)
    ref = _reference((B, C, L, xdt, bdt, "add"), x, br, w, b, scale, gres, gy, norm=False)
    _check("x_new", x_new, ref["x_new"], xdt, _tol_y(xdt))
    assert x.grad.stride() == x.stride() and torch.equal(x.grad, gres)             # dx is dres itself
    _check("dbranch", br.grad, ref["dbranch"], bdt, _tol_g(bdt))
    if scale is not None:
        z = B // 2
        assert torch.equal(x_new[z], x[z]) and not bool(br.grad[z].any())


@pytest.mark.parametrize("xdt,bdt", [(F32, BF16), (BF16, BF16)])
def test_strided_views_and_absent_gradients(xdt, bdt, cuda):
    """x a batch-strided slice of a larger buffer, branch a row slice with a token stride above C, the gradient of x_new
    arriving token-major; then each of the two incoming gradients absent."""
    from vivim_amd import layernorm as ln
    B, C, L = 2, 96, 200
    x0, br0, w, b, scale, gres, gy = _inputs(B, C, L, xdt, bdt, cuda, 11)
    big = torch.zeros(2 * B, C, L, dtype=xdt, device=cuda)
    big[::2] = x0.transpose(1, 2)
    x = big[::2].transpose(1, 2)
    wide = torch.zeros(B, L, C + 32, dtype=bdt, device=cuda)
    wide[..., :C] = br0
    br = wide[..., :C]
    assert x.stride(0) == 2 * C * L and br.stride(1) == C + 32 and ln.add_norm_supported(x, br, w)
    x.requires_grad_(True), br.requires_grad_(True), w.requires_grad_(True), b.requires_grad_(True)
    x_new, y = ln.add_layer_norm_cm(x, br, w, b, 1e-5, scale)
    assert x_new.stride() == (C * L, 1, L) and y.is_contiguous()
    gy = gy.to(y.dtype)
    gres_tm = gres.contiguous()                                                    # same values, token-major memory
    gx, gb, gw, gbias = torch.autograd.grad([x_new, y], [x, br, w, b], [gres_tm, gy], retain_graph=True)
    ref = _reference((B, C, L, xdt, bdt, "strided"), x, br, w, b, scale, gres, gy)
    _check("x_new", x_new, ref["x_new"], xdt, _tol_y(xdt))
    _check("y", y, ref["y"], y.dtype, _tol_y(y.dtype))
    _check("dx", gx, ref["dx"], xdt, _tol_g(xdt))
    _check("dbranch", gb, ref["dbranch"], bdt, _tol_g(bdt))
    _check("dweight", gw, ref["dw"], F32, 1e-4)
    _check("dbias", gbias, ref["db"], F32, 1e-4)
    assert gx.shape == x.shape and gx.stride(1) == 1                               # channel-major
    assert not bool(big[1::2].any()) and not bool(wide[..., C:].any())             # nothing written between the slices
    # only dres: dx = dres, dbranch = s * dres, no weight gradient
    gx, gb = torch.autograd.grad([x_new], [x, br], [gres], retain_graph=True)
    s = scale[:, None, None]
    assert torch.equal(gx, gres)
    _check("dbranch (dres only)", gb, s.double() * gres.double(), bdt, _tol_g(bdt))
    # only dy: the plain LayerNorm backward
    gx, gw = torch.autograd.grad([y], [x, w], [gy])
    x64 = x_new.detach().double().requires_grad_(True)
    w64 = w.detach().double().requires_grad_(True)
    F.layer_norm(x64, (C,), w64, b.detach().double(), 1e-5).backward(gy.double())
    _check("dx (dy only)", gx, x64.grad, xdt, _tol_g(xdt))
    _check("dweight (dy only)", gw, w64.grad, F32, 1e-4)


def test_unsupported_inputs(cuda):
    from vivim_amd import layernorm as ln
    x, br, w, b, _, _, _ = _inputs(2, 64, 256, BF16, BF16, cuda, 3)
    assert ln.add_norm_supported(x, br, w) and ln.add_norm_supported(x, br, None)
    assert not ln.add_norm_supported(x, br.float(), w)                              # a 16-bit stream with an f32 branch
    assert not ln.add_norm_supported(x, br.to(F16), w)
    assert not ln.add_norm_supported(x.contiguous(), br, w)                         # token-major x
    assert not ln.add_norm_supported(x, br.transpose(1, 2).contiguous().transpose(1, 2), w)    # channel-major branch
    assert not ln.add_norm_supported(x, br, w.to(BF16))
    big = _inputs(1, 1024, 64, F32, F32, cuda, 3)
    assert not ln.add_norm_supported(big[0], big[1], big[2])                        # > 512 channels
    odd = _inputs(1, 64, 36, BF16, BF16, cuda, 3)
    assert not ln.add_norm_supported(odd[0], odd[1], odd[2])                        # 36 tokens: not whole 16-byte pieces


def _run(layer, x):
    for p in layer.parameters():
        p.grad = None
    y = layer(x)
    y.square().mean().backward()
    return y.detach(), {n: p.grad.clone() for n, p in layer.named_parameters()}


def _pair(dim, cuda, drop_path=0.0, seed=5):
    """The same weights with the flag off and on."""
    from modeling.vivim import MambaLayer
    torch.manual_seed(seed)
    off = MambaLayer(dim, drop_path=drop_path).to(cuda)
    on = MambaLayer(dim, drop_path=drop_path, fused_add_norm=True).to(cuda)
    assert list(off.state_dict()) == list(on.state_dict())
    on.load_state_dict(off.state_dict())
    return off, on


def _count(monkeypatch):
    from vivim_amd import layernorm as ln
    calls = {"add_layer_norm_cm": 0, "add_cm": 0}
    for name in calls:
        real = getattr(ln, name)

        def counted(*a, _real=real, _name=name, **k):
            calls[_name] += 1
            return _real(*a, **k)
        monkeypatch.setattr(ln, name, counted)
    return calls


@pytest.mark.parametrize("drop_path,train", [(0.0, True), (0.1, False)])
def test_mamba_layer_flag_on_against_flag_off(drop_path, train, cuda, monkeypatch):
    off, on = _pair(64, cuda, drop_path)
    off.train(train), on.train(train)
    x = torch.randn(2, 64, 2, 32, 32, device=cuda)          # 4 096 tokens: layernorm.worthwhile's threshold
    calls = _count(monkeypatch)
    y0, g0 = _run(off, x)
    assert calls == {"add_layer_norm_cm": 0, "add_cm": 0}
    y1, g1 = _run(on, x)
    assert calls == {"add_layer_norm_cm": 1, "add_cm": 1}    # once per site
    assert y1.shape == y0.shape and y1.is_contiguous()
    e = rel_err(y1, y0)
    print(f"output: {e:.3e}")
    assert e < 1e-5
    assert set(g0) == set(g1)
    for n in g0:
        e = rel_err(g1[n], g0[n])
        print(f"{n}: {e:.3e}")
        assert e < 2e-4, n


def test_mamba_layer_train_drop_path_uses_the_scale(cuda, monkeypatch):
    """Training with DropPath on: both sites get a (B,) f32 scale of 0 or 1 / keep, and the module's own gradient flows."""
    from vivim_amd import layernorm as ln
    _, on = _pair(64, cuda, 0.5)
    on.train()
    seen = []
    for name in ("add_layer_norm_cm", "add_cm"):
        real = getattr(ln, name)
        monkeypatch.setattr(ln, name, lambda *a, _real=real: (seen.append(a[-1]), _real(*a))[1])
    x = torch.randn(8, 64, 2, 16, 16, device=cuda)
    _run(on, x)
    assert len(seen) == 2
    for s in seen:
        assert s.shape == (8,) and s.dtype == F32 and bool(((s == 0) | (s == 2.0)).all())


def test_mamba_layer_bf16_autocast(cuda, monkeypatch):
    """d0: what the fp32 summation order inside ONE norm kernel does to the layer (flag off, our kernel against ATen's).  The
    flag changes the same thing at two sites, so it may move the output by twice that."""
    off, on = _pair(64, cuda)
    x = torch.randn(2, 64, 2, 32, 32, device=cuda)

    def run(layer):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return _run(layer, x)
    y_off, g_off = run(off)
    calls = _count(monkeypatch)
    y_on, g_on = run(on)
    assert calls == {"add_layer_norm_cm": 1, "add_cm": 1}
    monkeypatch.setenv("VIVIM_NO_FUSED_LAYERNORM", "1")
    y_aten, g_aten = run(off)
    monkeypatch.delenv("VIVIM_NO_FUSED_LAYERNORM")
    d0, d1 = rel_err(y_off, y_aten), rel_err(y_on, y_off)
    print(f"output: d0 {d0:.3e}, fused against flag-off {d1:.3e}")
    for n in g_off:
        print(f"{n}: d0 {rel_err(g_off[n], g_aten[n]):.3e}, fused against flag-off {rel_err(g_on[n], g_off[n]):.3e}")
    assert d1 <= 2 * d0 + 1e-5


def test_deterministic_mode_keeps_the_flag_off_path(cuda, monkeypatch):
    _, on = _pair(64, cuda)
    x = torch.randn(2, 64, 2, 32, 32, device=cuda)
    calls = _count(monkeypatch)
    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        y1, g1 = _run(on, x)
        y2, g2 = _run(on, x)
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=prev_warn)
    assert calls == {"add_layer_norm_cm": 0, "add_cm": 0}
    assert torch.equal(y1, y2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n


@pytest.mark.parametrize("dim,shape,autocast", [(64, (1, 64, 1, 5, 8), True), (1024, (1, 1024, 2, 8, 8), False)])
def test_fallback_matches_flag_off_exactly(dim, shape, autocast, cuda, monkeypatch):
    """40 tokens under bf16 autocast (an op the kernels take, below layernorm.worthwhile) and 1 024 channels (above the
    kernels' 512): today's path, the same kernels in the same order.  The output is equal bit for bit; a parameter gradient
    is too unless the flag-off layer itself does not repeat it (float atomics in the scan's backward), and then it is
    within twice that layer's own run-to-run difference."""
    off, on = _pair(dim, cuda)
    x = torch.randn(*shape, device=cuda)

    def run(layer):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            return _run(layer, x)
    calls = _count(monkeypatch)
    y0, g0 = run(off)
    _, g0b = run(off)
    y1, g1 = run(on)
    assert calls == {"add_layer_norm_cm": 0, "add_cm": 0}
    assert torch.equal(y0, y1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]) or rel_err(g1[n], g0[n]) <= 2 * rel_err(g0b[n], g0[n]), n
