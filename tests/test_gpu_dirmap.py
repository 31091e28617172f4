"""GPU: the direction maps of csrc/dirmap.hip (vivim_amd/dirmap.py) in every branch of dir_dispatch, against index operations
on float64 copies of the rounded inputs (tests/v3_block_cases.py).

dir_dispatch takes the LDS-tile kernel when hw % E == 0 and 2 <= nf <= 16, E the element count of a 16-byte vector (4 fp32, 8
16-bit); a workgroup of it owns Q = 64 * E pixel positions.  Otherwise the element-wise kernel runs, 256 vectors per workgroup,
and walks the frames inside each vector.  The shapes below are written in terms of E so that every dtype reaches the same
branch, and every test asserts the branch its row claims, by dir_dispatch's rule.

    the stack (scatter, scale 1) is a permutation: torch.equal;
    every summing path (the stack's gradient, the combine) is (a + b + c) * scale in fp32, rounded once to the I/O type:
        |got - ref64| <= gamma(4) * (|a| + |b| + |c|) * scale + u_T * |ref64| * (1 + 2^-20)
      -- two fp32 adds, the rounded 1/3 and one multiply in any order, then one rounding to the I/O type; nothing measured;
    the combine's gradient is a scaled permutation: torch.equal to (g.float() * (1/3)).to(dtype), permuted."""
import pytest
import torch

import v3_block_cases as vc
from fp64_bounds import U_ROUND, elem_ratio, gamma, log_ratio

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _E(dtype):
    return 16 // torch.empty((), dtype=dtype).element_size()


# (B, D, nf, hw as a function of E, kernel, detail); detail: for the tile kernel (workgroups per (batch, channel), last piece
# partial); for the element-wise kernel (x-blocks, most frame boundaries inside one vector: 0 inside a frame, 1 a straddle,
# >= 2 several frames in one vector -- for fp32 and for the 16-bit types where they differ)
CASES = [
    ("tile_2wg_partial", 2, 3, 5, lambda E: 65 * E, "tile", (2, True)),
    ("tile_2wg_full", 1, 2, 2, lambda E: 128 * E, "tile", (2, False)),
    ("tile_nf16_full", 1, 2, 16, lambda E: 64 * E, "tile", (1, False)),
    ("tile_smallest", 1, 1, 2, lambda E: E, "tile", (1, True)),
    ("elem_nf17_inside", 1, 2, 17, lambda E: 16 * E, "elem", (2, {4: 0, 8: 0})),
    ("elem_straddle_hw5", 2, 3, 8, lambda E: 5, "elem", (1, {4: 1, 8: 2})),
    ("elem_straddle_hw6", 1, 2, 4, lambda E: 6, "elem", (1, {4: 1, 8: 1})),
    ("elem_frames_hw3", 1, 2, 8, lambda E: 3, "elem", (1, {4: 1, 8: 3})),
    ("elem_frames_hw1", 1, 1, 24, lambda E: 1, "elem", (1, {4: 3, 8: 7})),
    ("nf1", 2, 4, 1, lambda E: 64, "elem", (1, {4: 0, 8: 0})),
]
IDS = [c[0] for c in CASES]


def branch(E, nf, hw):
    """What dir_dispatch does with (E, nf, hw): (kernel, detail) as in CASES."""
    L = nf * hw
    if hw % E == 0 and 2 <= nf <= 16:
        Q = 64 * E
        return "tile", ((hw + Q - 1) // Q, hw % Q != 0)
    crossings = max((l0 + E - 1) // hw - l0 // hw for l0 in range(0, L, E))
    return "elem", ((L // E + 255) // 256, crossings)


def _shape(case, dtype):
    _, B, D, nf, hw_of, kernel, detail = case
    E = _E(dtype)
    hw = hw_of(E)
    assert (nf * hw) % E == 0                                           # what the entry point asks for
    want = (kernel, detail if kernel == "tile" else (detail[0], detail[1][E]))
    assert branch(E, nf, hw) == want, f"{case[0]}: dir_dispatch takes {branch(E, nf, hw)} for E = {E}, the table says {want}"
    if kernel == "elem" and detail[0] > 1:
        assert (nf * hw // E) % 256 != 0                                # the second x-block is a partial one
    return B, D, nf, hw, E


def _input(shape, dtype, gen, cuda, layout):
    """(B, C, L) values rounded to dtype; `inproj`: strides (L, B*L, 1) as in_proj's matmul leaves them, else contiguous."""
    B, C, L = shape
    if layout == "inproj":
        return torch.randn(C, B, L, generator=gen).to(dtype).to(cuda).transpose(0, 1)
    return torch.randn(B, C, L, generator=gen).to(dtype).to(cuda)


def _sum_bound(a, b, c, scale, dtype):
    """-> (ref64, bound) of (a + b + c) * scale computed in fp32 and rounded once to dtype; a, b, c float64, aligned."""
    ref = (a + b + c) * scale
    return ref, gamma(4) * (a.abs() + b.abs() + c.abs()) * scale + U_ROUND[dtype] * ref.abs() * (1 + 2.0 ** -20)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("layout", ["inproj", "contiguous"])
@pytest.mark.parametrize("halves", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stack_directions(case, halves, layout, dtype, cuda):
    """Forward: three bit-exact slices.  Backward: the sum of the three maps' inverses, within the summing bound."""
    from vivim_amd.dirmap import stack_directions
    B, D, nf, hw, E = _shape(case, dtype)
    L, C = nf * hw, 2 * D
    gen = torch.Generator().manual_seed(1000 * B + 10 * D + nf)
    xz = _input((B, C, L), dtype, gen, cuda, layout).requires_grad_(True)
    assert xz.stride() == ((L, B * L, 1) if layout == "inproj" else (C * L, L, 1))
    stk = stack_directions(xz, nf, halves)
    cs = C // halves
    assert stk.shape == (B, halves, 3, cs, L) and stk.dtype == dtype
    want = [t.reshape(B, halves, cs, L) for t in vc.map_stack(xz, nf)]
    got = stk.detach().double().cpu()
    for d, name in enumerate(("identity", "flip", "interleave")):
        assert torch.equal(got[:, :, d], want[d]), f"{case[0]}: direction {d} ({name}) is not the permutation of the input"
    w = torch.randn(B, halves, 3, cs, L, generator=gen).to(dtype).to(cuda)
    (gx,) = torch.autograd.grad(stk, xz, w)
    assert gx.shape == xz.shape and gx.dtype == dtype
    parts = vc.map_unstack(w[:, :, 0], w[:, :, 1], w[:, :, 2], nf)
    ref, bound = _sum_bound(*parts, 1.0, dtype)
    ratio = elem_ratio(gx.reshape(B, halves, cs, L), ref, bound)
    log_ratio(f"dirmap.stack_grad[{case[0]},halves={halves},{layout}]", dtype, (B, C, nf, hw), ratio)
    assert ratio <= 1.0, f"{case[0]}: stack gradient err / bound = {ratio:.3f}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("layout", ["inproj", "contiguous"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_combine_directions(case, layout, dtype, cuda):
    """Forward: (o + o_b.flip + o_s^-1) / 3 within the summing bound.  Backward: a bit-exact scaled permutation."""
    from vivim_amd.dirmap import combine_directions
    B, D, nf, hw, E = _shape(case, dtype)
    L = nf * hw
    gen = torch.Generator().manual_seed(2000 * B + 10 * D + nf)
    o3 = _input((B, 3 * D, L), dtype, gen, cuda, layout).view(B, 3, D, L).requires_grad_(True)
    y = combine_directions(o3, nf)
    assert y.shape == (B, D, L) and y.dtype == dtype
    assert y.stride() == (L, B * L, 1)              # (D, B, L) memory: its token-major transpose is out_proj's GEMM operand as it lies
    parts = vc.map_unstack(o3[:, 0], o3[:, 1], o3[:, 2], nf)
    ref, bound = _sum_bound(*parts, 1.0 / 3.0, dtype)
    ratio = elem_ratio(y, ref, bound)
    log_ratio(f"dirmap.combine[{case[0]},{layout}]", dtype, (B, D, nf, hw), ratio)
    assert ratio <= 1.0, f"{case[0]}: combine err / bound = {ratio:.3f}"
    gy = _input((B, D, L), dtype, gen, cuda, layout)
    (go,) = torch.autograd.grad(y, o3, gy)
    assert go.shape == o3.shape and go.dtype == dtype
    r = (gy.float() * (1.0 / 3.0)).to(dtype).cpu()
    got = go.cpu()
    assert torch.equal(got[:, 0], r) and torch.equal(got[:, 1], r.flip(-1))
    assert torch.equal(got[:, 2], vc.interleave(r, nf))


# ---- strides and stray writes, through the C ABI: valid calls whose destination has padding between its rows

STRIDE_CASES = [CASES[0], CASES[5]]                                     # one tile shape, one element-wise shape
SENTINEL = -7.0                                                         # exact in every dtype; compared bit for bit


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _launch(name, P, B, C, L, nf, csplit, dtype, flat_strides, stk_strides, src, dst, device):
    from vivim_amd import _lib
    P.batch, P.channels, P.seqlen, P.nframes, P.csplit, P.itype, P.scale = B, C, L, nf, csplit, _lib.ITYPE[dtype], 1.0
    P.flat_batch_stride, P.flat_c_stride = flat_strides
    P.stk_batch_stride, P.stk_half_stride, P.stk_dir_stride, P.stk_c_stride = stk_strides
    P.src, P.dst = src.data_ptr(), dst.data_ptr()
    assert all(s % (16 // src.element_size()) == 0 for s in (*flat_strides, *stk_strides))
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    _lib.launch(name, P, device)
    torch.cuda.synchronize()


def _padding_untouched(buf, shape, strides):
    """Every element of the 1-d `buf` outside its as_strided(shape, strides) payload still holds the sentinel's bits."""
    payload = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    payload.as_strided(shape, strides).fill_(True)
    assert int(payload.sum()) == torch.Size(shape).numel()              # the padded layout does not overlap itself
    pad = _bits(buf)[~payload]
    assert pad.numel() > 0
    return bool((pad == _bits(torch.full((1,), SENTINEL, dtype=buf.dtype, device=buf.device))).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", STRIDE_CASES, ids=[c[0] for c in STRIDE_CASES])
def test_scatter_into_padded_rows(case, dtype, cuda):
    """The stacked buffer's rows are L + 2E long, with padding after every direction, half and batch as well: the payload is
    the permutation and no padding element is written."""
    from vivim_amd import _lib
    B, D, nf, hw, E = _shape(case, dtype)
    L, C, halves = nf * hw, 2 * D, 2
    cs = C // halves
    gen = torch.Generator().manual_seed(31)
    flat = torch.randn(B, C, L, generator=gen).to(dtype).to(cuda)
    c_stride = L + 2 * E
    dir_stride = cs * c_stride + E
    half_stride = 3 * dir_stride + 2 * E
    batch_stride = halves * half_stride + 3 * E
    strides = (batch_stride, half_stride, dir_stride, c_stride, 1)
    shape = (B, halves, 3, cs, L)
    buf = torch.full((B * batch_stride,), SENTINEL, dtype=dtype, device=cuda)
    _launch("vivim_dir_scatter", _lib.DirParams(), B, C, L, nf, cs, dtype, (C * L, L), strides[:4], flat, buf, cuda)
    got = buf.as_strided(shape, strides).double().cpu()
    want = [t.reshape(B, halves, cs, L) for t in vc.map_stack(flat, nf)]
    for d in range(3):
        assert torch.equal(got[:, :, d], want[d]), f"direction {d}"
    assert _padding_untouched(buf, shape, strides)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", STRIDE_CASES, ids=[c[0] for c in STRIDE_CASES])
def test_gather_into_padded_rows(case, dtype, cuda):
    """The flat destination's rows are L + 2E long (and the batches padded): the payload is the sum within its bound and no
    padding element is written."""
    from vivim_amd import _lib
    B, D, nf, hw, E = _shape(case, dtype)
    L, C, halves = nf * hw, 2 * D, 2
    cs = C // halves
    gen = torch.Generator().manual_seed(37)
    stk = torch.randn(B, halves, 3, cs, L, generator=gen).to(dtype).to(cuda)
    c_stride = L + 2 * E
    batch_stride = C * c_stride + 3 * E
    buf = torch.full((B * batch_stride,), SENTINEL, dtype=dtype, device=cuda)
    _launch("vivim_dir_gather", _lib.DirParams(), B, C, L, nf, cs, dtype, (batch_stride, c_stride), stk.stride()[:4], stk, buf, cuda)
    shape, strides = (B, C, L), (batch_stride, c_stride, 1)
    parts = vc.map_unstack(stk[:, :, 0], stk[:, :, 1], stk[:, :, 2], nf)
    ref, bound = _sum_bound(*parts, 1.0, dtype)
    ratio = elem_ratio(buf.as_strided(shape, strides).reshape(B, halves, cs, L), ref, bound)
    log_ratio(f"dirmap.gather_padded[{case[0]}]", dtype, (B, C, nf, hw), ratio)
    assert ratio <= 1.0
    assert _padding_untouched(buf, shape, strides)
