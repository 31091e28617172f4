"""GPU: the one launch path of the binding (_lib.launch -> _lib.call).  The scan and conv1d wrappers, which used to enter
torch.cuda.device for every launch, give the same bits with a side stream current and with tensors that live on a device
other than the current one; profile_begin() records the four hot-path names alone and profile_begin(all_kernels=True) the
lean forward and the deterministic variants under their own names."""
import pytest
import torch

from vivim_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture
def det():
    """torch.use_deterministic_algorithms(True) for the test: the reduced gradients become comparable bit for bit."""
    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(prev, warn_only=prev_warn)


def _conv_inputs(dev):
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(1, 64, 64, generator=gen).to(torch.bfloat16).to(dev)
    dout = torch.randn(1, 64, 64, generator=gen).to(torch.bfloat16).to(dev)
    return x, torch.randn(64, 4, generator=gen).to(dev), torch.randn(64, generator=gen).to(dev), dout


def _conv(x, w, b, dout):
    """-> [out, dx, dweight, dbias] of causal_conv1d_fwd / _bwd (batch 1, dim 64, seqlen 64, width 4, bf16, SiLU)."""
    import causal_conv1d_cuda as cc
    return [cc.causal_conv1d_fwd(x, w, b, True)] + cc.causal_conv1d_bwd(x, w, b, dout, None, True)


def _scan_inputs(dev):
    gen = torch.Generator().manual_seed(4)
    bf = lambda *shape: torch.randn(*shape, generator=gen).to(torch.bfloat16).to(dev)                # noqa: E731
    t = dict(u=bf(1, 64, 64), delta=bf(1, 64, 64) * 0.5, B=bf(1, 1, 16, 64), C=bf(1, 1, 16, 64), z=bf(1, 64, 64),
             A=-torch.rand(64, 16, generator=gen).to(dev) - 0.5, D=torch.randn(64, generator=gen).to(dev),
             delta_bias=torch.randn(64, generator=gen).to(dev) * 0.1)
    return t, bf(1, 64, 64)


def _scan(t, dout):
    """-> [out, du, ddelta, dz, dA, dB, dC, dD, ddelta_bias, lean out] of selective_scan_fn forward + backward and of its
    no-grad call (batch 1, dim 64, dstate 16, seqlen 64, bf16, with z)."""
    from mamba_ssm.ops.selective_scan_interface import selective_scan_fn
    names = ("u", "delta", "z", "A", "B", "C", "D", "delta_bias")
    q = {k: t[k].detach().clone().requires_grad_(True) for k in names}
    out = selective_scan_fn(q["u"], q["delta"], q["A"], q["B"], q["C"], q["D"], q["z"], q["delta_bias"], True)
    out.backward(dout)
    with torch.no_grad():
        lean = selective_scan_fn(t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["z"], t["delta_bias"], True)
    return [out.detach()] + [q[k].grad for k in names] + [lean]


def _assert_equal(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.device == b.device and torch.equal(a, b), f"{what}: tensor {i} differs"


@pytest.mark.parametrize("op", ["conv1d", "scan"])
def test_side_stream_gives_the_same_bits(op, cuda, det):
    inputs, run = (_conv_inputs(cuda), _conv) if op == "conv1d" else (_scan_inputs(cuda), _scan)
    want = run(*inputs)
    if op == "scan":
        assert torch.equal(want[0], want[-1]), "the lean forward is the full forward's bits"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = run(*inputs)
    torch.cuda.current_stream().wait_stream(side)
    _assert_equal(got, want, op + " on a side stream")


@pytest.mark.parametrize("op", ["conv1d", "scan"])
def test_tensors_off_the_current_device(op, det):
    """The one branch of _lib.launch the rest of the suite never takes: cuda:0 is current, the tensors live on cuda:1.  The
    deterministic conv1d backward allocates its slot workspace there too."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    dev = torch.device("cuda:1")
    torch.cuda.set_device(0)
    inputs, run = (_conv_inputs(dev), _conv) if op == "conv1d" else (_scan_inputs(dev), _scan)
    with torch.cuda.device(1):
        want = run(*inputs)
    assert torch.cuda.current_device() == 0
    got = run(*inputs)
    assert torch.cuda.current_device() == 0
    assert all(g.device == dev for g in got)
    _assert_equal(got, want, op + " on cuda:1 with cuda:0 current")


def test_profile_records(cuda):
    x, w, b, dout = _conv_inputs(cuda)
    t, sdout = _scan_inputs(cuda)
    _lib.profile_begin()
    try:
        _conv(x, w, b, dout)
        _scan(t, sdout)                                                      # its lean call is not a hot-path name
    finally:
        rec = _lib.profile_end()
    assert sorted(r[0] for r in rec) == sorted(_lib._PROFILED) and len(rec) == 4
    assert all(r[1] > 0 for r in rec)

    P = _lib.ConvBwdParams()                                                 # what algorithmic_bytes reads of the conv1d struct
    P.f.batch, P.f.dim, P.f.seqlen, P.f.width, P.f.itype = 1, 64, 64, 4, _lib.BF16
    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    _lib.profile_begin(all_kernels=True)
    try:
        _conv(x, w, b, dout)                                                 # the default backward
        _scan(t, sdout)                                                      # full forward, backward, lean forward
        torch.use_deterministic_algorithms(True)
        _conv(x, w, b, dout)                                                 # the deterministic backward
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=prev_warn)
        rec = _lib.profile_end()
    nbytes = {}
    for name, n, _ in rec:
        nbytes.setdefault(name, []).append(n)
    assert len(nbytes["vivim_selective_scan_fwd_lean"]) == 1 and nbytes["vivim_selective_scan_fwd_lean"][0] > 0
    assert len(nbytes["vivim_causal_conv1d_bwd_det"]) == 1 and len(nbytes["vivim_causal_conv1d_bwd"]) == 1
    want = _lib.algorithmic_bytes("vivim_causal_conv1d_bwd", P)
    assert nbytes["vivim_causal_conv1d_bwd_det"][0] == nbytes["vivim_causal_conv1d_bwd"][0] == want > 0
