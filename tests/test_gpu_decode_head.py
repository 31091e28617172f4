"""GPU: the fused eval-mode decode head (csrc/decode_head.hip, vivim_amd/decode_head.py) against an fp64 restatement from the
very same inputs, elementwise, in fp32 / fp16 / bf16; bit-repeatability across streams; and the head inside Vivim against the
stock head and an fp64 copy of it.

Reference.  Per map and axis the tap matrix M (n_out x n_in) is built from the definition (r = float(n_in) / float(n_out),
src = max(0, r (o + 0.5) - 0.5), i0 = int(src), i1 = i0 + (i0 < n_in - 1), l1 = src - i0, l0 = 1 - l1) in torch fp32 on the CPU
and placed in fp64; everything after is fp64 on the maps already rounded to the I/O dtype:
    pre[k] = bias[k] + sum_s (M_h m_s M_w^T)[k],  A[k] = |bias[k]| + sum_s (|M_h| |m_s| |M_w|^T)[k],  h = max(0, pre),
    want[c] = b[c] + sum_k w_out[c][k] h[k].

Bound, elementwise, u = 2^-24:
    |got - want| <= (K + 20) u (|b[c]| + sum_k |w_out[c][k]| A[k]) + half a unit in the last place of the output type at want.
Where it comes from, for this kernel's order of operations: a tap passes through at most four roundings on its way into h (two
products or fmas per axis) and h collects at most four maps and the bias, one rounding each: |h - h_exact| <= 9 u A to first
order, and the ReLU is 1-Lipschitz.  The class sum is a dot product of K terms: one rounding per product, and whatever the
order -- here each lane adds its E channels per chunk in sequence and a six-step butterfly joins the lanes -- every partial sum
is a sum of distinct terms, no term passes through more than K - 1 real additions (adding a lane's exact zero rounds nothing)
and its error is at most (K - 1) u sum|w h|.  One more rounding adds b.  (9 + 1 + K - 1 + 1) u = (K + 10) u, second-order terms
included well below (K + 20) u.  A wrong tap, a missed channel or a dropped map is an error of order one.
The worst share of the bound and the norm-wise error go to the parity log that conftest.py keeps."""
import copy
import functools
import os

import pytest
import torch

from conftest import _PARITY_LOG, DT

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MANT = {torch.float32: 24, torch.float16: 11, torch.bfloat16: 8}        # significand bits: half an ulp at x is 2^(floor(log2|x|) - bits)

# name: (N, K, C, (out_h, out_w), map sizes)
CASES = {
    "ratios": (2, 768, 3, (16, 16), ((16, 16), (8, 8), (4, 4), (2, 2))),            # the workload's ratios
    "odd": (1, 768, 3, (13, 19), ((13, 19), (7, 10), (4, 5), (1, 1))),              # non-integer ratios, a single-pixel map
    "k72_c8": (3, 72, 8, (9, 5), ((9, 5), (5, 3), (3, 2), (2, 1))),                 # vector path, partly filled wave, largest C
    "k50_c1": (2, 50, 1, (6, 7), ((6, 7), (3, 4))),                                 # element path for every dtype
    "k7_same": (2, 7, 2, (5, 5), ((5, 5),)),                                        # nothing is upsampled
    "tile_edges": (1, 64, 3, (17, 65), ((17, 65), (9, 33), (5, 17), (3, 9))),       # one past the 8 x 8 tile on both axes
}
DTYPES = ("fp32", "fp16", "bf16")


def tap_matrix(n_in, n_out):
    """The (n_out, n_in) matrix of one axis: the definition in torch fp32 on the CPU, placed in fp64."""
    r = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    o = torch.arange(n_out, dtype=torch.float32)
    src = torch.clamp(r * (o + 0.5) - 0.5, min=0.0)
    i0 = src.to(torch.int64)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    l1 = src - i0.to(torch.float32)
    l0 = 1.0 - l1
    assert src.dtype == l0.dtype == torch.float32 and int(i1.max()) <= n_in - 1
    rows = torch.arange(n_out)
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    M.index_put_((rows, i0), l0.double(), accumulate=True)
    M.index_put_((rows, i1), l1.double(), accumulate=True)
    return M


def _half_ulp(want, dtype):
    _, e = torch.frexp(want.abs())                          # |want| = m 2^e, m in [0.5, 1): floor(log2 |want|) = e - 1
    return torch.where(want == 0, torch.zeros_like(want), torch.ldexp(torch.ones_like(want), e - 1 - MANT[dtype]))


def _reference(maps, bias, w_out, b_out, size):
    """fp64 `want` and the elementwise bound, from CPU tensors (the maps already rounded to their dtype)."""
    K, dtype = maps[0].shape[3], maps[0].dtype
    pre = bias.double()[None, None, None, :]
    A = bias.double().abs()[None, None, None, :]
    for m in maps:
        Mh, Mw = tap_matrix(m.shape[1], size[0]), tap_matrix(m.shape[2], size[1])
        pre = pre + torch.einsum("oh,nhwk,pw->nopk", Mh, m.double(), Mw)
        A = A + torch.einsum("oh,nhwk,pw->nopk", Mh.abs(), m.double().abs(), Mw.abs())
    b = torch.zeros(w_out.shape[0], dtype=torch.float64) if b_out is None else b_out.double()
    want = torch.einsum("ck,nopk->ncop", w_out.double(), pre.clamp_min(0.0)) + b[None, :, None, None]
    scale = torch.einsum("ck,nopk->ncop", w_out.double().abs(), A) + b.abs()[None, :, None, None]
    return want, (K + 20) * U * scale + _half_ulp(want, dtype)


@functools.lru_cache(maxsize=None)
def case(name, dt):
    """Inputs (rounded to the dtype) and the fp64 reference of one case, computed once and shared; nobody writes to them."""
    N, K, C, size, sizes = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    maps = [torch.randn(N, h, w, K, generator=g).to(DT[dt]) for h, w in sizes]
    bias, w_out, b_out = torch.randn(K, generator=g), torch.randn(C, K, generator=g) / K ** 0.5, torch.randn(C, generator=g)
    want, bound = _reference(maps, bias, w_out, b_out, size)
    return dict(maps=maps, bias=bias, w_out=w_out, b_out=b_out, size=size, want=want, bound=bound)


def _check(test, dt, got, want, bound):
    """Log the worst share of the bound and the norm-wise error, then assert the bound elementwise."""
    err = (got.detach().double().cpu() - want).abs()
    share = float((err / bound.clamp_min(1e-300)).max())
    rel = float((got.detach().double().cpu() - want).norm() / want.norm().clamp_min(1e-30))
    try:
        os.makedirs(os.path.dirname(_PARITY_LOG), exist_ok=True)
        with open(_PARITY_LOG, "a") as f:
            f.write(f"{test}\tlogits\t{dt}\tshape={tuple(got.shape)}\trel_err={rel:.3e}\tmax_abs={float(err.max()):.3e}"
                    f"\tmax_err_over_bound={share:.3e}\n")
    except OSError:
        pass
    print(f"{test} {dt}: norm-wise {rel:.3e}, max|err| {float(err.max()):.3e}, worst share of the bound {share:.3e}")
    bad = err > bound
    assert not bool(bad.any()), (f"{test} ({dt}): {int(bad.sum())} of {bad.numel()} logits outside the bound, worst {share:.3e} x, "
                                 f"first at {bad.nonzero()[0].tolist()}")


def _run(ref, cuda, **kw):
    from vivim_amd import fused_decode_head
    b_out = ref["b_out"]
    return fused_decode_head([m.to(cuda) for m in ref["maps"]], ref["bias"].to(cuda), ref["w_out"].to(cuda),
                             None if b_out is None else b_out.to(cuda), ref["size"], **kw)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_fp64(name, dt, cuda):
    from vivim_amd import decode_head
    ref = case(name, dt)
    N, K, C, size, _ = CASES[name]
    assert decode_head.supported([m.to(cuda) for m in ref["maps"]], ref["bias"].to(cuda), ref["w_out"].to(cuda),
                                 ref["b_out"].to(cuda), size)
    got = _run(ref, cuda)
    assert got.shape == (N, C, *size) and got.dtype == DT[dt] and got.is_contiguous()
    assert torch.isfinite(got.float()).all()
    _check(f"decode_head[{name}]", dt, got, ref["want"], ref["bound"])


@pytest.mark.parametrize("dt", DTYPES)
def test_batch_slices_and_an_odd_element_offset(dt, cuda):
    """Case "ratios" with every map a batch slice of a wider tensor, map 2 starting one element into its storage (no 16-byte
    access is aligned there: the element path) and the logits written into a batch slice whose padding stays untouched."""
    from vivim_amd import fused_decode_head
    ref = case("ratios", dt)
    N, K, C, size, _ = CASES["ratios"]
    maps = []
    for s, m in enumerate(ref["maps"]):
        n_img, off = m[0].numel(), (1 if s == 2 else 0)
        buf = torch.full((N, n_img + 8 + off), float("nan"), dtype=m.dtype, device=cuda)
        v = buf[:, off:off + n_img].view(m.shape)
        v.copy_(m)
        assert v.stride(0) > n_img and v.data_ptr() % 16 == (off * m.element_size()) % 16
        maps.append(v)
    n_out = C * size[0] * size[1]
    obuf = torch.full((N, n_out + 5), 7.0, dtype=DT[dt], device=cuda)
    out = obuf[:, :n_out].view(N, C, *size)
    got = fused_decode_head(maps, ref["bias"].to(cuda), ref["w_out"].to(cuda), ref["b_out"].to(cuda), size, out=out)
    assert got.data_ptr() == out.data_ptr() and bool((obuf[:, n_out:] == 7.0).all())
    _check("decode_head[slices]", dt, got, ref["want"], ref["bound"])


@pytest.mark.parametrize("with_b_out", (True, False))
@pytest.mark.parametrize("dt", DTYPES)
def test_everything_clipped_leaves_b_out(dt, with_b_out, cuda):
    """bias = -1e4: every hidden value is clipped by the ReLU, the logits are b_out rounded to the dtype exactly (zeros without)."""
    ref = dict(case("ratios", dt))
    N, K, C, size, _ = CASES["ratios"]
    ref["bias"] = torch.full((K,), -1e4)
    if not with_b_out:
        ref["b_out"] = None
    got = _run(ref, cuda)
    want = torch.zeros(C) if ref["b_out"] is None else ref["b_out"]
    assert torch.equal(got.cpu(), want.to(DT[dt])[None, :, None, None].expand(N, C, *size))


@pytest.mark.parametrize("dt", ("fp32", "bf16"))
def test_repeatable_on_any_stream(dt, cuda):
    ref = case("ratios", dt)
    a = _run(ref, cuda)
    junk = torch.full((16 << 20,), float("nan"), device=cuda)       # the next buffers come back from the allocator full of NaN
    del junk
    b = _run(ref, cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = _run(ref, cuda)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(a, b) and torch.equal(a, c)


# ---- the head inside Vivim ------------------------------------------------------------------------------------------------------
DIMS = (64, 128, 320, 512)


def _build_head(cuda):
    """A Vivim (with the edge head) on a one-block-per-stage SegFormer from a local config, BatchNorm statistics and projection
    biases randomised; its fp64 copy; and four random encoder states of 2 x 2 frames."""
    from transformers import SegformerConfig, SegformerForSemanticSegmentation
    from vivim_amd.decode_head import _projections
    from vivim_amd.vivim import Vivim
    torch.manual_seed(41)
    cfg = SegformerConfig(num_channels=3, num_encoder_blocks=4, depths=[1, 1, 1, 1], sr_ratios=[8, 4, 2, 1],
                          hidden_sizes=list(DIMS), patch_sizes=[7, 3, 3, 3], strides=[4, 2, 2, 2],
                          num_attention_heads=[1, 2, 5, 8], mlp_ratios=[4, 4, 4, 4], decoder_hidden_size=768, num_labels=150)
    model = Vivim(in_chans=3, out_chans=3, depths=[1, 1, 1, 1], backbone=SegformerForSemanticSegmentation(cfg), with_edge=True,
                  fused_decode_head=True)
    g = torch.Generator().manual_seed(42)
    bn = model.decoder.batch_norm
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(768, generator=g))
        bn.running_var.copy_(torch.rand(768, generator=g) * 1.5 + 0.5)
        bn.weight.copy_(torch.randn(768, generator=g))
        bn.bias.copy_(torch.randn(768, generator=g))
        for proj in _projections(model.decoder):
            proj.bias.copy_(torch.randn(768, generator=g))
    model = model.to(cuda).eval()
    states = tuple(torch.randn(4, c, s, s, generator=g).to(cuda) for c, s in zip(DIMS, (16, 8, 4, 2)))
    return model, states


@pytest.fixture(scope="module")
def head(cuda):
    return _build_head(cuda)


def _decode(model, states, fused, bz=2, nf=2):
    model.fused_decode_head = fused
    try:
        return model.decode(states, bz, nf)
    finally:
        model.fused_decode_head = True


def _fp64_stock(model, states):
    ref = copy.deepcopy(model).double()
    ref.fused_decode_head = False
    with torch.no_grad():
        return ref.decode(tuple(x.double() for x in states), 2, 2)


def _rel(got, want):
    return float((got.double() - want).norm() / want.norm())


def _calls(fn):
    """fn() and the names of the C-ABI calls it made (the _lib profile hook)."""
    from vivim_amd import _lib
    _lib.profile_begin(all_kernels=True)
    try:
        out = fn()
    finally:
        names = [r[0] for r in _lib.profile_end()]
    return out, names


def _same_format(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    for fmt in (torch.contiguous_format, torch.channels_last):
        assert a.is_contiguous(memory_format=fmt) == b.is_contiguous(memory_format=fmt)


def test_head_fp32_against_fp64(head):
    model, states = head
    want = _fp64_stock(model, states)
    with torch.no_grad():
        fused, names = _calls(lambda: _decode(model, states, True))
        stock, names_stock = _calls(lambda: _decode(model, states, False))
    assert names.count("vivim_decode_head_fwd") == 1 and "vivim_decode_head_fwd" not in names_stock
    e_fused, e_stock = _rel(fused, want), _rel(stock, want)
    print(f"decode head fp32 against fp64: fused {e_fused:.3e}, stock {e_stock:.3e}")
    assert e_fused < 1e-3 and e_stock < 1e-3
    _same_format(fused, stock)


def test_head_fp16_autocast_against_fp64(head):
    model, states = head
    want = _fp64_stock(model, states)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        fused = _decode(model, states, True)
        stock = _decode(model, states, False)
    e_fused, e_stock = _rel(fused, want), _rel(stock, want)
    print(f"decode head fp16 autocast against fp64: fused {e_fused:.3e}, stock {e_stock:.3e}")
    assert fused.dtype == torch.float16
    assert e_fused < 1e-3
    _same_format(fused, stock)


def test_head_bf16_autocast_is_no_worse_than_the_stock_head(head):
    """The logits' own bf16 rounding is about 1e-3: the fused head's error against fp64 must not exceed the stock head's, measured
    in the same run."""
    model, states = head
    want = _fp64_stock(model, states)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        fused = _decode(model, states, True)
        stock = _decode(model, states, False)
    e_fused, e_stock = _rel(fused, want), _rel(stock, want)
    print(f"decode head bf16 autocast against fp64: fused {e_fused:.3e}, stock {e_stock:.3e}")
    assert fused.dtype == torch.bfloat16
    assert e_fused <= e_stock
    _same_format(fused, stock)


def test_whole_forward_bf16(head, cuda):
    """Vivim.forward in eval at (1, 2, 3, 64, 64) under bf16 autocast, the switch on and off on the same weights: against the
    fp64 stock head on the same encoder states (upsampled in fp64) the fused logits are no further off than the stock ones; the
    edge maps, which the switch does not touch, are bit-equal."""
    import torch.nn.functional as F
    model, _ = head
    x = torch.randn(1, 2, 3, 64, 64, generator=torch.Generator().manual_seed(43)).to(cuda)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        (logits_on, edge_on), names = _calls(lambda: model(x))
        model.fused_decode_head = False
        try:
            logits_off, edge_off = model(x)
        finally:
            model.fused_decode_head = True
        outs = model.encoder(x)
    assert names.count("vivim_decode_head_fwd") == 1
    want = F.interpolate(_fp64_stock_nf(model, outs), size=(64, 64), mode="bilinear", align_corners=False)
    e_on, e_off = _rel(logits_on, want), _rel(logits_off, want)
    print(f"whole forward bf16 against the fp64 head: switch on {e_on:.3e}, off {e_off:.3e}")
    assert logits_on.shape == logits_off.shape == (2, 3, 64, 64) and logits_on.dtype == logits_off.dtype
    assert e_on <= e_off
    assert torch.equal(edge_on, edge_off)


def _fp64_stock_nf(model, outs):
    ref = copy.deepcopy(model).double()
    ref.fused_decode_head = False
    with torch.no_grad():
        return ref.decode(tuple(o.double() for o in outs), 1, 2)


@pytest.fixture
def det():
    """torch.use_deterministic_algorithms(True), strict, for the test; restored afterwards whatever happens."""
    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(prev, warn_only=prev_warn)


def test_grad_or_train_mode_take_the_stock_path(head, det):
    """With grad enabled (eval) and in train(), switch on and off give equal bits with equal RNG state, the kernel is not
    called, and backward works.  Equal bits need a stock head that repeats itself: without the deterministic flag MIOpen's
    fp32 linear_fuse convolution does not on this device (two identical calls of the stock head differ from linear_fuse on, with
    or without grad), so the comparison runs under the strict flag, with the upsampling through csrc/upsample.hip because
    ATen's upsampling backward raises there (as tests/test_gpu_upsample.py runs the head)."""
    model, states = head
    model = copy.deepcopy(model)                            # train mode moves BatchNorm's running statistics
    model.fused_upsample = True
    try:
        for train in (False, True):
            model.train(train)
            outs = []
            for fused in (True, False):
                torch.manual_seed(7)
                xs = tuple(x.clone().requires_grad_(True) for x in states)
                y, names = _calls(lambda: _decode(model, xs, fused))
                assert "vivim_decode_head_fwd" not in names and y.requires_grad
                model.zero_grad(set_to_none=True)
                y.float().square().mean().backward()
                assert all(x.grad is not None and torch.isfinite(x.grad).all() for x in xs)
                assert model.decoder.linear_fuse.weight.grad is not None
                outs.append(y.detach())
            assert torch.equal(outs[0], outs[1]), f"train={train}"
    finally:
        model.eval()


def test_an_optimizer_step_reaches_the_next_eval_call(head):
    model, states = head
    model = copy.deepcopy(model)
    with torch.no_grad():
        before = _decode(model, states, True)
    opt = torch.optim.SGD(model.decoder.parameters(), lr=0.05)
    model.train()
    _decode(model, tuple(x.clone() for x in states), False).square().mean().backward()
    opt.step()
    model.eval()
    want = _fp64_stock(model, states)
    with torch.no_grad():
        fused = _decode(model, states, True)
        stock = _decode(model, states, False)
    e_fused, e_stock, moved = _rel(fused, want), _rel(stock, want), _rel(fused, before.double())
    print(f"after an optimizer step: fused {e_fused:.3e}, stock {e_stock:.3e} against fp64; the logits moved by {moved:.3e}")
    assert moved > 1e-2                                        # the step did change the head (and BatchNorm's statistics)
    assert e_fused < 1e-3 and e_stock < 1e-3
