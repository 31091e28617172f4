"""GPU: under torch.use_deterministic_algorithms the selective-scan backward takes vivim_selective_scan_bwd_det: every
backward family (lanes = tokens with 8 / 4 waves, generic, lanes = states first / second generation) matches the CPU
oracle and gives the same bits on every repeat, on a second stream and with a NaN-filled workspace."""
import pytest
import torch

from test_gpu_kernels import BWD_VARIANTS, FWD_VARIANTS, _check_scan, _rand_scan

pytestmark = pytest.mark.gpu

# (forward that writes the checkpoints the family reads, backward family)
FAMILIES = {"tokens_w8": ("nsplit_k8", "fast_w8"), "tokens_w4": ("nsplit_k8", "fast_w4"), "generic": ("generic", "generic"),
            "states1": ("states", "states"), "states2": ("channels", "states2")}


@pytest.fixture
def det():
    """torch.use_deterministic_algorithms(True) for the test, restored afterwards whatever happens."""
    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(prev, warn_only=prev_warn)


@pytest.fixture
def pin():
    from vivim_amd import _lib
    L = _lib.lib()
    prev = []

    def set_(fwd, bwd):
        prev.append((L.vivim_set_tuning(0, fwd), L.vivim_set_tuning(1, bwd)))

    yield set_
    if prev:
        L.vivim_set_tuning(0, prev[0][0])
        L.vivim_set_tuning(1, prev[0][1])


def _grads(ss, t, x, out):
    dz = torch.empty_like(t["z"])
    g = ss.bwd(t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["z"], t["delta_bias"], t["dout"], x, out, dz,
               t["softplus"], False)
    return [v.clone() for v in g[:7]] + [dz.clone()]


def _repeats_equal(ss, t, n):
    res = ss.fwd(t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["z"], t["delta_bias"], t["softplus"])
    out, x = res[0], res[1]
    first = _grads(ss, t, x, out)
    names = ["du", "ddelta", "dA", "dB", "dC", "dD", "ddelta_bias", "dz"]
    side = torch.cuda.Stream()
    for i in range(n):
        if i % 2:                                 # the workspace comes back from the caching allocator full of NaN
            junk = torch.full((64 << 20,), float("nan"), device=t["u"].device)
            del junk
        if i % 3 == 2:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                g = _grads(ss, t, x, out)
            torch.cuda.current_stream().wait_stream(side)
        else:
            g = _grads(ss, t, x, out)
        for name, a, b in zip(names, first, g):
            assert torch.equal(a, b), f"repeat {i}: {name} differs"


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("dstate", [16, 64])
def test_det_scan_backward(family, dtype, dstate, cuda, det, pin):
    import selective_scan_cuda as ss
    if family == "states2" and dstate != 16:
        pytest.skip("the second-generation lanes = states kernel is dstate 16 only")
    fwd, bwd = FAMILIES[family]
    pin(FWD_VARIANTS[fwd], BWD_VARIANTS[bwd])
    gen = torch.Generator().manual_seed(dstate * 7 + len(family))
    t = _rand_scan(gen, 4, 128, dstate, 8192, 1, dtype, cuda, init="module")
    _check_scan(t, ss)                            # oracle: norm-wise AND the reference's rtol / atol
    _repeats_equal(ss, t, 20)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_det_scan_backward_constant_bc(dtype, cuda, det, pin):
    """Constant B / C (dim, dstate): generic family, per-step adds folded in LDS, one slot per batch element."""
    import selective_scan_cuda as ss
    pin(FWD_VARIANTS["generic"], BWD_VARIANTS["generic"])
    gen = torch.Generator().manual_seed(5)
    t = _rand_scan(gen, 4, 128, 16, 2048, 1, dtype, cuda, init="module")
    t["B"] = torch.randn(128, 16, generator=gen).to(cuda)
    t["C"] = torch.randn(128, 16, generator=gen).to(cuda)
    _check_scan(t, ss)
    _repeats_equal(ss, t, 20)


def test_det_scan_long_rows_auto(cuda, det, pin):
    """The automatic plan at 20480 tokens (many segments) with batch 4."""
    import selective_scan_cuda as ss
    pin(0, 0)
    gen = torch.Generator().manual_seed(9)
    t = _rand_scan(gen, 4, 128, 16, 20480, 1, torch.bfloat16, cuda, strided=True, init="module")
    _check_scan(t, ss)
    _repeats_equal(ss, t, 20)


def _same_over_repeats(run, n):
    first = [g.clone() for g in run()]
    for i in range(n):
        if i % 2:
            junk = torch.full((64 << 20,), float("nan"), device="cuda")
            del junk
        for j, (a, b) in enumerate(zip(first, run())):
            assert torch.equal(a, b), f"repeat {i}: tensor {j} differs"
    return first


@pytest.mark.parametrize("width", [2, 3, 4])
@pytest.mark.parametrize("has_bias", [True, False])
@pytest.mark.parametrize("channel_last", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_det_conv1d_backward(width, has_bias, channel_last, dtype, cuda, det):
    """dx (into a caller view), dweight, dbias: equal over 20 repeats and close to the default path's result."""
    import causal_conv1d_cuda as cc
    g = torch.Generator().manual_seed(width)
    B, D, L = 4, 192, 8192
    x = torch.randn(B, D, L, generator=g).to(cuda, dtype)
    dout = torch.randn(B, D, L, generator=g).to(cuda, dtype)
    if channel_last:
        x = x.transpose(1, 2).contiguous().transpose(1, 2)
        dout = dout.transpose(1, 2).contiguous().transpose(1, 2)
    w = (torch.randn(D, width, generator=g) * 0.3).to(cuda)
    b = (torch.randn(D, generator=g) * 0.1).to(cuda) if has_bias else None
    big = torch.empty(B, D + 8, L, dtype=dtype, device=cuda) if not channel_last else \
        torch.empty(B, L, D + 8, dtype=dtype, device=cuda).transpose(1, 2)
    dx_view = big[:, 4:4 + D]

    def run():
        dx, dw, db = cc.causal_conv1d_bwd(x, w, b, dout, dx_view, True)
        return [dx_view.clone(), dw] + ([db] if has_bias else [])

    got = _same_over_repeats(run, 20)
    torch.use_deterministic_algorithms(False)
    want = run()
    torch.use_deterministic_algorithms(True)
    for a, e in zip(got, want):
        torch.testing.assert_close(a.float(), e.float(), rtol=1e-4 if dtype == torch.float32 else 2e-2, atol=1e-3)


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_det_dwconv_wgrad(D, dtype, cuda, det):
    from vivim_amd.dwconv import depthwise_conv_tokens
    g = torch.Generator().manual_seed(D)
    C, H, W, B = 128, 32, 32, 4
    x = torch.randn(B, D * H * W, C, generator=g).to(cuda, dtype).requires_grad_(True)
    k = (C, 1, 3, 3) if D == 1 else (C, 1, 3, 3, 3)
    wt = (torch.randn(*k, generator=g) * 0.2).to(cuda).requires_grad_(True)
    bias = torch.randn(C, generator=g).to(cuda).requires_grad_(True)
    dy = torch.randn(B, D * H * W, C, generator=g).to(cuda, dtype)

    def run():
        x.grad = wt.grad = bias.grad = None
        depthwise_conv_tokens(x, wt, bias, D, H, W).backward(dy)
        return [x.grad, wt.grad, bias.grad]

    got = _same_over_repeats(run, 20)
    torch.use_deterministic_algorithms(False)
    want = run()
    torch.use_deterministic_algorithms(True)
    for a, e in zip(got, want):
        torch.testing.assert_close(a.float(), e.float(), rtol=1e-3 if dtype == torch.float32 else 2e-2, atol=1e-2)


@pytest.mark.parametrize("autocast", [False, True])
def test_det_mamba_v3_bit_identical(autocast, cuda, det):
    from mamba_ssm import Mamba
    torch.manual_seed(0)
    m = Mamba(d_model=64, d_state=16, d_conv=4, expand=2, bimamba_type="v3", nframes=5).to(cuda)
    x = torch.randn(2, 5 * 16 * 16, 64, device=cuda, requires_grad=True)

    def run():
        m.zero_grad(set_to_none=True)
        x.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            y = m(x)
        y.float().square().mean().backward()
        return [x.grad] + [p.grad for p in m.parameters()]

    _same_over_repeats(run, 3)


def test_det_mamba_layer_bit_identical(cuda, det):
    from modeling.vivim import MambaLayer
    torch.manual_seed(0)
    layer = MambaLayer(dim=64).to(cuda)
    x = torch.randn(2, 64, 5, 16, 16, device=cuda, requires_grad=True)

    def run():
        layer.zero_grad(set_to_none=True)
        x.grad = None
        layer(x).square().mean().backward()
        return [x.grad] + [p.grad for p in layer.parameters() if p.grad is not None]

    _same_over_repeats(run, 3)
