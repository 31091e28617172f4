"""GPU: vivim_amd.bilinear_upsample (csrc/upsample.hip) against the definition, elementwise, forward and backward, in fp32 /
fp16 / bf16 and both layouts; the transpose identity; no launch at equal size; bit-repeatability under the strict
deterministic flag, alone and inside the decode head; and no write outside y / dx (VIVIM_GUARD child).

Reference.  The per-axis tap matrices M_h (out_h x in_h), M_w are built from the definition (r = float(n_in) / float(n_out),
src = max(0, r (o + 0.5) - 0.5), i0 = int(src), i1 = i0 + (i0 < n_in - 1), l1 = src - i0, l0 = 1 - l1) in torch fp32 on the CPU
and placed in fp64; R_fwd = M_h x M_w^T on the input already rounded to the I/O dtype, R_bwd = M_h^T g M_w, both in fp64.  The
restatement is itself cross-checked against fp64 F.interpolate and its autograd at 1e-4 max|x| (ATen's CPU path forms the taps
in fp64: agreement is about 1e-6).

Bounds, elementwise, u = 2^-23, n = max(in_h, in_w), T = 4 ceil(out_h / in_h) ceil(out_w / in_w), rho = one unit in the last
place of the output type (0 / 2^-10 / 2^-8):
    forward   |y - R|      <= 8 u max|x| + 4 n u max|x| + rho |R|      four products and three adds; one ulp of src (fused
                                                                       against unfused tap arithmetic); the output rounding
    backward  |dx - R_bwd| <= (T + 4) u S + 4 n u G + rho |R_bwd|      S = |M_h|^T |g| |M_w|, G = (M_h > 0)^T |g| (M_w > 0)
A wrong tap, an off-by-one window or a missed edge is an error of order |x| / scale: four orders above these.
The measured maxima go to the parity log that conftest.py keeps, next to ATen's device result; ATen's forward is asserted at twice the
forward bound, its 16-bit backward (16-bit atomics) is only logged."""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import _PARITY_LOG, DT, ROOT

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
RHO = {torch.float32: 0.0, torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -8}

# name: (N, C, (in_h, in_w), (out_h, out_w))
CASES = {
    "one_pixel": (2, 3, (1, 1), (4, 4)),             # single input pixel: every tap clamps
    "tiny_frac": (2, 3, (2, 3), (7, 5)),             # non-integer scale, tiny
    "equal_h": (1, 5, (3, 3), (3, 8)),               # equal size on one axis
    "just_above_1": (2, 3, (7, 5), (9, 11)),
    "x8": (1, 8, (5, 7), (40, 56)),                  # the stage-3 ratio
    "x33": (2, 3, (3, 2), (100, 67)),                # scale 33.3, output width not a multiple of 64
    "wide_rows": (1, 2, (4, 70), (16, 300)),         # rows wider than one tile
    "logits": (2, 3, (64, 64), (256, 256)),          # the logits' own ratio and size
}
CL_ONLY = {
    "c768": (2, 768, (8, 8), (64, 64)),              # bf16 only: vector path and plane count
    "c6": (1, 6, (5, 7), (20, 28)),                  # C that does not fill a 16-byte vector
    "c13": (1, 13, (5, 7), (20, 28)),
}
ALL = dict(CASES, **CL_ONLY)
PARAMS = ([(name, layout, dt) for name in CASES for layout in ("planes", "cl") for dt in ("fp32", "fp16", "bf16")]
          + [("c768", "cl", "bf16")] + [(name, "cl", dt) for name in ("c6", "c13") for dt in ("fp32", "fp16", "bf16")])


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


@functools.lru_cache(maxsize=None)
def reference(name, dt):
    """Inputs (rounded to the dtype) and fp64 references of one case, computed once and shared; nobody writes to them."""
    N, C, (H, W), (OH, OW) = ALL[name]
    dtype = DT[dt]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(N, C, H, W, generator=g).to(dtype)
    go = torch.randn(N, C, OH, OW, generator=g).to(dtype)
    Mh, Mw = tap_matrix(H, OH), tap_matrix(W, OW)
    x64, g64 = x.double(), go.double()
    R = torch.einsum("oh,nchw,pw->ncop", Mh, x64, Mw)
    Rb = torch.einsum("oh,ncop,pw->nchw", Mh, g64, Mw)
    S = torch.einsum("oh,ncop,pw->nchw", Mh.abs(), g64.abs(), Mw.abs())
    G = torch.einsum("oh,ncop,pw->nchw", (Mh > 0).double(), g64.abs(), (Mw > 0).double())
    n, T = max(H, W), 4 * math.ceil(OH / H) * math.ceil(OW / W)
    xmax = float(x64.abs().max())
    fwd_bound = (8 + 4 * n) * U * xmax + RHO[dtype] * R.abs()
    bwd_bound = (T + 4) * U * S + 4 * n * U * G + RHO[dtype] * Rb.abs()
    # the restatement against ATen's fp64 CPU path, loosely: a wrong restatement must not hide a wrong kernel
    xa = x64.clone().requires_grad_(True)
    ya = F.interpolate(xa, size=(OH, OW), mode="bilinear", align_corners=False)
    ya.backward(g64)
    assert float((ya.detach() - R).abs().max()) <= 1e-4 * xmax
    assert float((xa.grad - Rb).abs().max()) <= 1e-4 * float(g64.abs().max())
    return dict(x=x, go=go, R=R, Rb=Rb, S=S, fwd_bound=fwd_bound, bwd_bound=bwd_bound, T=T, size=(OH, OW))


def _log(test, name, dtype, got, want, bound):
    err = (got.detach().double().cpu() - want).abs()
    mx, ratio = float(err.max()), float((err / bound.clamp_min(1e-300)).max())
    try:
        os.makedirs(os.path.dirname(_PARITY_LOG), exist_ok=True)
        with open(_PARITY_LOG, "a") as f:
            f.write(f"{test}\t{name}\t{str(dtype).replace('torch.', '')}\tshape={tuple(got.shape)}\tmax_abs={mx:.3e}"
                    f"\tmax_err_over_bound={ratio:.3e}\n")
    except OSError:
        pass
    print(f"{test} {name} {dtype}: max|err| {mx:.3e}, max err / bound {ratio:.3e}")
    return err


def _within(err, bound, what, factor=1.0):
    bad = err > factor * bound
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, worst "
                                 f"{float((err / bound.clamp_min(1e-300)).max()):.3e} x, first at {bad.nonzero()[0].tolist()}")


def _to_layout(t, layout, cuda):
    t = t.to(cuda)
    return t.contiguous(memory_format=torch.channels_last) if layout == "cl" else t.contiguous()


def _run(fn, x, go):
    x = x.detach().requires_grad_(True)
    y = fn(x)
    y.backward(go)
    return y.detach(), x.grad


@pytest.mark.parametrize("name,layout,dt", PARAMS)
def test_values_and_gradients(name, layout, dt, cuda):
    from vivim_amd import bilinear_upsample, upsample
    ref, dtype = reference(name, dt), DT[dt]
    size = ref["size"]
    x, go = _to_layout(ref["x"], layout, cuda), _to_layout(ref["go"], layout, cuda)
    assert upsample.supported(x, size)
    aten = lambda t: F.interpolate(t, size=size, mode="bilinear", align_corners=False)   # noqa: E731
    y, dx = _run(lambda t: bilinear_upsample(t, size), x, go)
    ya, dxa = _run(aten, x, go)
    assert y.dtype == dx.dtype == dtype and y.shape == ya.shape and dx.shape == x.shape
    for fmt in (torch.contiguous_format, torch.channels_last):                 # ATen's memory formats (a size of 1 leaves its stride free)
        assert y.is_contiguous(memory_format=fmt) == ya.is_contiguous(memory_format=fmt)
        assert dx.is_contiguous(memory_format=fmt) == dxa.is_contiguous(memory_format=fmt)
    assert torch.isfinite(y.float()).all() and torch.isfinite(dx.float()).all()
    test = f"upsample[{name}-{layout}]"
    err_y = _log(test, "y", dtype, y, ref["R"], ref["fwd_bound"])
    err_dx = _log(test, "dx", dtype, dx, ref["Rb"], ref["bwd_bound"])
    err_ya = _log(test, "y_aten", dtype, ya, ref["R"], ref["fwd_bound"])
    _log(test, "dx_aten", dtype, dxa, ref["Rb"], ref["bwd_bound"])           # 16-bit atomics in ATen: logged, not asserted
    _within(err_y, ref["fwd_bound"], f"{test} y ({dtype})")
    _within(err_dx, ref["bwd_bound"], f"{test} dx ({dtype})")
    _within(err_ya, ref["fwd_bound"], f"{test} ATen's y ({dtype})", factor=2.0)


def _odd_view(t, layout):
    """The same values as a view one element into a larger buffer: misaligned for every 16-byte access."""
    N, C, H, W = t.shape
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    if layout == "cl":
        v = buf[1:].view(N, H, W, C).permute(0, 3, 1, 2)
    else:
        v = buf[1:].view(N, C, H, W)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.stride() == t.stride()
    return v


@pytest.mark.parametrize("layout,dt", [("cl", "bf16"), ("planes", "fp32")])
def test_odd_element_offset_takes_element_accesses(layout, dt, cuda):
    from vivim_amd import bilinear_upsample
    ref, dtype = reference("x8", dt), DT[dt]
    size = ref["size"]
    x, go = _to_layout(ref["x"], layout, cuda), _to_layout(ref["go"], layout, cuda)
    y0, dx0 = _run(lambda t: bilinear_upsample(t, size), x, go)               # aligned: C = 8 bf16 fills one 16-byte vector
    y1, dx1 = _run(lambda t: bilinear_upsample(t, size), _odd_view(x, layout), _odd_view(go, layout))
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    _within(_log(f"upsample_odd[{layout}]", "y", dtype, y1, ref["R"], ref["fwd_bound"]), ref["fwd_bound"], "y at an odd offset")
    _within(_log(f"upsample_odd[{layout}]", "dx", dtype, dx1, ref["Rb"], ref["bwd_bound"]), ref["bwd_bound"], "dx at an odd offset")


@pytest.mark.parametrize("layout", ["planes", "cl"])
def test_under_autocast_the_dtypes_are_atens(layout, cuda):
    """upsample_bilinear2d is on autocast's fp32 list: a bf16 input gives an fp32 output and a bf16 gradient, here as in ATen."""
    from vivim_amd import bilinear_upsample
    ref = reference("x8", "bf16")
    size = ref["size"]
    x, go = _to_layout(ref["x"], layout, cuda), _to_layout(ref["go"], layout, cuda).float()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y, dx = _run(lambda t: bilinear_upsample(t, size), x, go)
        ya, dxa = _run(lambda t: F.interpolate(t, size=size, mode="bilinear", align_corners=False), x, go)
    assert y.dtype == ya.dtype == torch.float32 and dx.dtype == dxa.dtype == torch.bfloat16
    bound = (8 + 4 * 7) * U * float(ref["x"].double().abs().max()) + 0.0 * ref["R"]       # fp32 output: rho = 0; n = 7
    _within(_log(f"upsample_autocast[{layout}]", "y", torch.float32, y, ref["R"], bound), bound, "y under autocast")
    _within(_log(f"upsample_autocast[{layout}]", "dx", torch.bfloat16, dx, ref["Rb"], ref["bwd_bound"]), ref["bwd_bound"],
            "dx under autocast")


def _recorded(fn):
    """fn() and the names of the C-ABI calls it made (the _lib profile hook)."""
    from vivim_amd import _lib
    _lib.profile_begin(all_kernels=True)
    try:
        out = fn()
    finally:
        names = [r[0] for r in _lib.profile_end()]
    return out, names


@pytest.mark.parametrize("layout", ["planes", "cl"])
def test_equal_size_launches_nothing(layout, cuda):
    from vivim_amd import bilinear_upsample
    x = _to_layout(torch.randn(2, 8, 5, 7).to(torch.bfloat16), layout, cuda)
    go = _to_layout(torch.randn(2, 8, 5, 7).to(torch.bfloat16), layout, cuda)
    bigger = _to_layout(torch.randn(2, 8, 10, 7).to(torch.bfloat16), layout, cuda)
    (y, dx), names_equal = _recorded(lambda: _run(lambda t: bilinear_upsample(t, (5, 7)), x, go))
    _, names_up = _recorded(lambda: _run(lambda t: bilinear_upsample(t, (10, 7)), x, bigger))
    assert not [n for n in names_equal if n.startswith("vivim_upsample")], names_equal
    assert names_up == ["vivim_upsample_bilinear2d_fwd", "vivim_upsample_bilinear2d_bwd"]      # the hook does see them
    assert torch.equal(y, x) and y.data_ptr() != x.data_ptr() and y.stride() == x.stride()
    assert torch.equal(dx, go)


@pytest.mark.parametrize("name,layout", [("x33", "planes"), ("just_above_1", "cl")])
def test_transpose_identity_fp32(name, layout, cuda):
    """<y(x), g> and <x, dx(g)> agree to (T + 8) u sum|x| S: forward and backward share one tap function."""
    from vivim_amd import bilinear_upsample
    ref = reference(name, "fp32")
    x, go = _to_layout(ref["x"], layout, cuda), _to_layout(ref["go"], layout, cuda)
    y, dx = _run(lambda t: bilinear_upsample(t, ref["size"]), x, go)
    a = float((y.double().cpu() * ref["go"].double()).sum())
    b = float((dx.double().cpu() * ref["x"].double()).sum())
    tol = (ref["T"] + 8) * U * float((ref["x"].double().abs() * ref["S"]).sum())
    print(f"transpose[{name}-{layout}]: <y, g> = {a:.9e}, <x, dx> = {b:.9e}, |difference| {abs(a - b):.3e}, tolerance {tol:.3e}")
    assert abs(a - b) <= tol


@pytest.fixture
def det():
    """torch.use_deterministic_algorithms(True), strict, for the test; restored afterwards whatever happens."""
    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(prev, warn_only=prev_warn)


@pytest.mark.parametrize("name,layout,dt", [("x8", "planes", "bf16"), ("x33", "planes", "fp32"), ("c768", "cl", "bf16")])
def test_repeatable_under_the_strict_flag(name, layout, dt, cuda, det):
    from vivim_amd import bilinear_upsample
    ref = reference(name, dt)
    x, go = _to_layout(ref["x"], layout, cuda), _to_layout(ref["go"], layout, cuda)
    run = lambda: _run(lambda t: bilinear_upsample(t, ref["size"]), x, go)      # noqa: E731
    y0, dx0 = run()
    _within((dx0.double().cpu() - ref["Rb"]).abs(), ref["bwd_bound"], "dx under the strict flag")
    side = torch.cuda.Stream()
    for i in range(20):
        if i % 2:                                  # the next buffers come back from the caching allocator full of NaN
            junk = torch.full((16 << 20,), float("nan"), device=cuda)
            del junk
        if i % 3 == 2:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                y, dx = run()
            torch.cuda.current_stream().wait_stream(side)
        else:
            y, dx = run()
        assert torch.equal(y, y0) and torch.equal(dx, dx0), f"repeat {i} differs"


@pytest.fixture(scope="module")
def head(cuda):
    """A Vivim on a one-block-per-stage SegFormer from a local config, and the four feature maps of a 64 x 64 clip of 2 frames."""
    from transformers import SegformerConfig, SegformerForSemanticSegmentation
    from vivim_amd.vivim import Vivim
    torch.manual_seed(11)
    cfg = SegformerConfig(num_channels=3, num_encoder_blocks=4, depths=[1, 1, 1, 1], sr_ratios=[8, 4, 2, 1],
                          hidden_sizes=[64, 128, 320, 512], patch_sizes=[7, 3, 3, 3], strides=[4, 2, 2, 2],
                          num_attention_heads=[1, 2, 5, 8], mlp_ratios=[4, 4, 4, 4], decoder_hidden_size=768, num_labels=150)
    model = Vivim(in_chans=3, out_chans=3, depths=[1, 1, 1, 1], backbone=SegformerForSemanticSegmentation(cfg),
                  fused_upsample=True).to(cuda).train()
    g = torch.Generator().manual_seed(12)
    feats = [torch.randn(2, c, s, s, generator=g).to(cuda) for c, s in ((64, 16), (128, 8), (320, 4), (512, 2))]
    go = torch.randn(2, 3, 64, 64, generator=g).to(cuda)
    return model, feats, go


def _head_step(model, feats, go):
    torch.manual_seed(5)                           # the per-map dropout coin flips (CPU RNG) and the dropout masks
    model.zero_grad(set_to_none=True)
    xs = [f.clone().requires_grad_(True) for f in feats]
    low = model.decode(tuple(xs), 1, 2)
    out = model._upsample(low, (64, 64))
    out.backward(go)
    grads = [x.grad for x in xs] + [p.grad.clone() for p in model.parameters() if p.grad is not None]
    return out.detach(), low.detach(), grads


def test_decode_head_is_repeatable_under_the_strict_flag(head, det):
    model, feats, go = head
    assert model.fused_upsample and model.training
    out0, _, grads0 = _head_step(model, feats, go)          # no RuntimeError: ATen's upsample backward would raise here
    assert len(grads0) > 4 and all(torch.isfinite(g).all() for g in grads0)
    for i in range(2):
        out, _, grads = _head_step(model, feats, go)
        assert torch.equal(out, out0), f"run {i + 1}: output differs"
        for j, (a, b) in enumerate(zip(grads0, grads)):
            assert torch.equal(a, b), f"run {i + 1}: gradient {j} differs"


def test_decode_head_matches_aten(head):
    """fused_upsample=False, flag off: the same module's outputs within twice the forward bound of the final upsample."""
    model, feats, go = head
    assert not torch.are_deterministic_algorithms_enabled()
    out1, low1, _ = _head_step(model, feats, go)
    model.fused_upsample = False
    try:
        out0, low0, _ = _head_step(model, feats, go)
    finally:
        model.fused_upsample = True
    xmax = float(low0.abs().max())
    bound = 2 * ((8 + 4 * 16) * U * xmax)                    # fp32: rho = 0; n = 16
    err_low, err = float((low1 - low0).abs().max()), float((out1 - out0).abs().max())
    print(f"decode head fused against ATen: max|d logits at 16 x 16| {err_low:.3e}, max|d output| {err:.3e}, bound {bound:.3e}, "
          f"max|logits| {xmax:.3e}")
    assert err <= bound


CHILD = r"""
import torch
from vivim_amd import _lib, bilinear_upsample
assert _lib.GUARD
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
n = 0
for (N, C, H, W, OH, OW) in ((2, 3, 3, 2, 100, 67), (1, 2, 4, 70, 16, 300), (1, 13, 5, 7, 20, 28), (2, 768, 8, 8, 64, 64),
                             (2, 3, 1, 1, 4, 4), (1, 5, 3, 3, 3, 3)):
    for dt in (torch.float32, torch.bfloat16):
        for fmt in (torch.contiguous_format, torch.channels_last):
            x = torch.randn(N, C, H, W, generator=g).to(dev).to(dt).contiguous(memory_format=fmt).requires_grad_(True)
            go = torch.randn(N, C, OH, OW, generator=g).to(dev).to(dt).contiguous(memory_format=fmt)
            y = bilinear_upsample(x, (OH, OW))
            y.backward(go)
            _lib.check_guards("upsample")
            assert torch.isfinite(y.float()).all() and torch.isfinite(x.grad.float()).all()
            n += 1
print("GUARD_OK", n)
"""


def test_writes_stay_inside_y_and_dx_under_guard(cuda):
    env = dict(os.environ, VIVIM_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GUARD_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
