"""GPU: the slot invariant of the deterministic backward kernels (csrc/det.cuh) -- every slot element det_reduce reads was written by
exactly one workgroup, for every shape -- at the shapes of tests/det_cases.py.  Every case asserts, in this order:
  1. parity with the reference the default path is held to, at the same figures: the C oracle for the scan (_check_scan) and the
     causal conv1d (test_conv_vs_oracle's), the fp64 convolution and its rounding-error bound for the depthwise conv;
  2. the same bits on three repeats whose slot workspace starts out full of NaN, 3e38 and -3e38 in turn: an unwritten slot
     element changes the result or makes it non-finite;
  3. scan only: the pinned family ran (its slot layout differs from the generic fallback's in size), and the call's workspace is
     never larger than what the shape-level query promises."""
import pytest
import torch

import det_cases as dc
import fp64_bounds as fb
from conftest import CONV_CLOSE, check_close, rel_err
from oracle import cpu_oracle
from test_gpu_deterministic import FAMILIES, det, pin  # noqa: F401  (det, pin: fixtures)
from test_gpu_kernels import BWD_VARIANTS, FWD_VARIANTS, _check_scan, _rand_scan, _round, _tol

pytestmark = pytest.mark.gpu

POISONS = (float("nan"), 3e38, -3e38)
GRADS = ["du", "ddelta", "dA", "dB", "dC", "dD", "ddelta_bias", "dz"]


class _Spy:
    """Stands in for _lib.workspace while a test runs: every slot workspace a deterministic call asks for is handed over full of
    `fill`, and the query, its params and its answer are kept."""

    def __init__(self, inner):
        self.inner, self.fill, self.calls = inner, POISONS[0], []

    def __call__(self, query, params, device):
        n, ws = self.inner(query, params, device)
        if "_det_" in query:
            self.calls.append((query, params, n))
            if ws is not None:
                ws.view(torch.float32).fill_(self.fill)
        return n, ws


@pytest.fixture
def spy(monkeypatch):
    from vivim_amd import _lib
    s = _Spy(_lib.workspace)
    monkeypatch.setattr(_lib, "workspace", s)
    return s


def _poison(spy, fill, nbytes):
    """The `junk` of test_gpu_deterministic._repeats_equal: a freed block larger than the call's workspace, full of `fill`, for the
    caching allocator to hand back; the spy fills the workspace itself with the same value, wherever it comes from."""
    spy.fill = fill
    junk = torch.full((nbytes // 4 + (1 << 20),), fill, device="cuda")
    del junk


def _same_bits(spy, run, nbytes, names):
    """run() after each poison of POISONS: every tensor finite, and bit-identical between the three."""
    first = None
    for fill in POISONS:
        _poison(spy, fill, nbytes)
        got = [None if g is None else g.clone() for g in run()]
        for name, g in zip(names, got):
            assert g is None or bool(torch.isfinite(g).all()), f"{name} is not finite after a workspace full of {fill}"
        if first is None:
            first = got
        for name, a, b in zip(names, first, got):
            assert (a is None and b is None) or torch.equal(a, b), f"{name} differs after a workspace full of {fill}"
    return first


# ------------------------------------------------------------------ selective scan

_problems = {}            # case name -> (tensors, oracle forward, oracle backward): computed once, never written to
_generic_bytes = {}       # case name -> slot workspace bytes of the generic family on that problem


def _problem(name, dev):
    if name not in _problems:
        c = dc.SCAN_CASES[name]
        gen = torch.Generator().manual_seed(sum(map(ord, name)))
        t = _rand_scan(gen, c.batch, c.dim, c.dstate, c.seqlen, c.groups, c.dtype, dev, strided=c.strided, init=c.init, **c.opts)
        if c.strided:                                  # (the stride of a batch axis of size 1 is whatever torch makes it)
            assert t["u"].stride()[1:] == (c.batch * c.seqlen, 1)
        fwd = cpu_oracle.selective_scan_fwd(t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["z"], t["delta_bias"], t["softplus"])
        bwd = cpu_oracle.selective_scan_bwd(t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["z"], t["delta_bias"], t["dout"],
                                            t["softplus"])
        _problems[name] = (t, fwd, bwd)
    return _problems[name]


def _scan_grads(ss, t):
    res = ss.fwd(t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["z"], t["delta_bias"], t["softplus"])
    out, x = res[0], res[1]

    def run():
        dz = torch.empty_like(t["z"]) if t["z"] is not None else None
        g = ss.bwd(t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["z"], t["delta_bias"], t["dout"], x,
                   out if t["z"] is not None else None, dz, t["softplus"], False)
        return list(g[:7]) + [dz]
    return run


def _scan_call_fits_shape(spy):
    """include/vivim_hip.h: the slots of the family a call's pointers select are never more than the shape-level size."""
    from vivim_amd import _lib
    calls = [c for c in spy.calls if c[0] == "vivim_scan_bwd_det_call_workspace_bytes"]
    assert calls, "the backward did not take the deterministic entry point"
    for _, P, n in calls:
        assert 0 < n <= _lib.lib().vivim_scan_bwd_det_workspace_bytes(P.f)


def _det_bytes_of(ss, t, pin, family):
    fwd, bwd = FAMILIES[family]
    pin(FWD_VARIANTS[fwd], BWD_VARIANTS[bwd])
    _scan_grads(ss, t)()
    return ss.last_workspace_bytes["bwd_det"], ss.last_workspace_bytes["bwd"]


def _states_slot_floats(c, det_bytes, seg_bytes):
    """What a lanes = states call's slot workspace holds beyond its dA / dD / dbias slots (one of dim * (dstate + 2) floats per (batch,
    segment)), in floats.  The segment count is read off the segment scratch the same plan asks for (batch * dim * segments *
    (2 dstate + 1) floats, none for one segment)."""
    segs = seg_bytes // (4 * c.batch * c.dim * (2 * c.dstate + 1)) if seg_bytes else 1
    return det_bytes // 4 - c.batch * segs * c.dim * (c.dstate + 2)


@pytest.mark.parametrize("family,name", [(f, n) for f in FAMILIES for n in dc.SCAN_FAMILY_CASES[f]])
def test_det_scan_edge_shapes(family, name, cuda, det, pin, spy):
    import selective_scan_cuda as ss
    c = dc.SCAN_CASES[name]
    fwd, bwd = FAMILIES[family]
    pin(FWD_VARIANTS[fwd], BWD_VARIANTS[bwd])
    t, ofwd, obwd = _problem(name, cuda)
    _check_scan(t, ss, ofwd, obwd)                                      # 1. the oracle, at the default tolerances
    nbytes, seg_bytes = ss.last_workspace_bytes["bwd_det"], ss.last_workspace_bytes["bwd"]
    _same_bits(spy, _scan_grads(ss, t), nbytes, GRADS)                  # 2. poisoned slots
    _scan_call_fits_shape(spy)                                          # 3. the family that ran
    if family == "generic":
        _generic_bytes[name] = nbytes
        return
    if name not in _generic_bytes:
        _generic_bytes[name] = _det_bytes_of(ss, t, pin, "generic")[0]
    assert nbytes != _generic_bytes[name], f"{family} fell back to the generic kernel at {name}"
    if family.startswith("states"):                                     # dB / dC slots exactly where a group has > 2 workgroups
        slots = c.states_bpg if c.states_bpg > 2 else 0
        assert _states_slot_floats(c, nbytes, seg_bytes) == 2 * slots * c.batch * c.groups * c.dstate * c.seqlen


@pytest.mark.parametrize("family", ["states1", "states2"])
def test_det_scan_states_slots_add_to_the_size(family, cuda, det, pin):
    """208 = 3 x 64 + 16 channels make four lanes = states workgroups per group, 128 make two: the slot workspace of the first
    exceeds the second's by more than its own dA / dD / dbias slots, i.e. it holds dB / dC slots and the second does not."""
    import selective_scan_cuda as ss
    sizes = {}
    for name in ("slotted_ragged", "pair_whole"):
        sizes[name] = _det_bytes_of(ss, _problem(name, cuda)[0], pin, family)
    c = dc.SCAN_CASES["slotted_ragged"]
    (big, seg_bytes), (small, _) = sizes["slotted_ragged"], sizes["pair_whole"]
    assert big - small > 4 * (big // 4 - _states_slot_floats(c, big, seg_bytes))
    assert _states_slot_floats(c, big, seg_bytes) == 2 * 4 * c.batch * c.dstate * c.seqlen
    assert _states_slot_floats(dc.SCAN_CASES["pair_whole"], small, sizes["pair_whole"][1]) == 0


@pytest.mark.parametrize("batch,dim,dstate,seqlen,dtype", dc.CONST_BC_CASES)
def test_det_scan_constant_bc_edge_shapes(batch, dim, dstate, seqlen, dtype, cuda, det, pin, spy):
    """Constant B / C of shape (dim, dstate): per-step adds folded in LDS, one (dim, dstate) slot per batch element."""
    import selective_scan_cuda as ss
    pin(FWD_VARIANTS["generic"], BWD_VARIANTS["generic"])
    gen = torch.Generator().manual_seed(dim + seqlen)
    t = _rand_scan(gen, batch, dim, dstate, seqlen, 1, dtype, cuda, init="module")
    t["B"] = torch.randn(dim, dstate, generator=gen).to(cuda)
    t["C"] = torch.randn(dim, dstate, generator=gen).to(cuda)
    _check_scan(t, ss)
    _same_bits(spy, _scan_grads(ss, t), ss.last_workspace_bytes["bwd_det"], GRADS)
    _scan_call_fits_shape(spy)


# ------------------------------------------------------------------ causal conv1d

def _conv_check(cc, spy, x, w, b, dout, dx_view, silu, dtype):
    rdx, rdw, rdb = cpu_oracle.causal_conv1d_bwd(x, w, b, dout, silu)

    def run():
        dx, dw, db = cc.causal_conv1d_bwd(x, w, b, dout, dx_view, silu)
        return [dx, dw, db]

    spy.calls.clear()
    dx, dw, db = run()
    assert [q for q, _, _ in spy.calls] == ["vivim_causal_conv1d_bwd_det_workspace_bytes"]
    check_close("conv_dx", dx, _round(rdx, dtype), dtype, CONV_CLOSE, _tol(dtype))     # the figures of test_conv_vs_oracle
    assert rel_err(dw, rdw) < 1e-4
    if b is not None:
        assert rel_err(db, rdb) < 1e-4
    else:
        assert db is None
    _same_bits(spy, run, spy.calls[0][2], ["dx", "dweight", "dbias"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=fb.name)
@pytest.mark.parametrize("batch,dim,seqlen,width,layout", dc.CONV_CASES)
def test_det_conv1d_edge_shapes(batch, dim, seqlen, width, layout, dtype, cuda, det, spy):
    import causal_conv1d_cuda as cc
    g = torch.Generator().manual_seed(dim * 7 + seqlen + width)
    dxz = dx_view = None
    if layout == "slice":
        x = torch.randn(batch, dim + 32, seqlen, generator=g).to(dtype).to(cuda)[:, 16:16 + dim]
        assert not x.is_contiguous()
    elif layout == "xz":
        xz = torch.randn(2 * dim, batch, seqlen, generator=g).to(dtype).to(cuda).transpose(0, 1)
        x = xz[:, :dim]
        assert x.stride() == (seqlen, batch * seqlen, 1)
        dxz = torch.full_like(xz, 7.0)
        dx_view = dxz[:, :dim]
    else:
        x = torch.randn(batch, dim, seqlen, generator=g).to(dtype).to(cuda)
    dout = torch.randn(batch, dim, seqlen, generator=g).to(dtype).to(cuda)
    w = torch.randn(dim, width, generator=g).to(cuda)
    bias = torch.randn(dim, generator=g).to(cuda)
    for has_bias, silu in dc.CONV_OPTIONS:
        _conv_check(cc, spy, x, w, bias if has_bias else None, dout, dx_view, silu, dtype)
        if dxz is not None:
            assert bool((dxz[:, dim:] == 7.0).all())                    # the other half of the caller's buffer is untouched


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=fb.name)
@pytest.mark.parametrize("batch,dim,seqlen,width,layout", dc.CONV_CL_CASES)
def test_det_conv1d_channel_last_edge_shapes(batch, dim, seqlen, width, layout, dtype, cuda, det, spy):
    import causal_conv1d_cuda as cc
    g = torch.Generator().manual_seed(dim * 5 + seqlen + width)
    if layout == "slice":
        x = torch.randn(batch, seqlen, dim + 3, generator=g).to(dtype).to(cuda)[:, :, 1:dim + 1].transpose(1, 2)
        assert x.stride(2) == dim + 3
    else:
        x = torch.randn(batch, seqlen, dim, generator=g).to(dtype).to(cuda).transpose(1, 2)
    assert x.shape == (batch, dim, seqlen) and x.stride(1) == 1
    dout = torch.randn(batch, seqlen, dim, generator=g).to(dtype).to(cuda).transpose(1, 2)
    w = torch.randn(dim, width, generator=g).to(cuda)
    bias = torch.randn(dim, generator=g).to(cuda)
    for has_bias, silu in dc.CONV_OPTIONS:
        _conv_check(cc, spy, x, w, bias if has_bias else None, dout, None, silu, dtype)


# ------------------------------------------------------------------ depthwise-conv weight gradient

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=fb.name)
@pytest.mark.parametrize("B,C,D,H,W,has_bias,k3", [c + (k3,) for c in dc.DWCONV_CASES for k3 in (False, True) if k3 or c[2] == 1])
def test_det_dwconv_wgrad_edge_shapes(B, C, D, H, W, has_bias, k3, dtype, cuda, det, spy):
    """dx, dweight and dbias per element within the fp64 bound of tests/fp64_bounds.py (err / bound <= 1, as test_gpu_dwconv.py), with
    3 x 3 x 3 taps and, on one frame, 3 x 3 taps.  A channel count the forward and dx kernels do not take goes to the weight-gradient
    entry point alone."""
    from vivim_amd import dwconv
    gen = torch.Generator().manual_seed(B * 100 + C + D * H * W)
    L = D * H * W
    x = torch.randn(B, L, C, generator=gen).to(dtype)
    w = torch.randn(*((C, 1, 3, 3, 3) if k3 else (C, 1, 3, 3)), generator=gen) * 0.3
    bias = torch.randn(C, generator=gen) if has_bias else None
    dy = torch.randn(B, L, C, generator=gen).to(dtype)
    ref, bound = fb.dwconv_reference(x, w, bias, dy, (D, H, W))
    xd, wd, dyd = x.to(cuda), w.to(cuda), dy.to(cuda)
    whole_op = dwconv.supported(xd, wd)
    assert whole_op == (C % (16 // x.element_size()) == 0)

    def run():
        if not whole_op:
            wt = dwconv._taps(wd)
            acc = dwconv._run_wgrad(xd, dyd, wt, (D, H, W), has_bias)
            return [None, acc[:wt.shape[0] * C].view(wt.shape[0], C).t().reshape(w.shape), acc[wt.shape[0] * C:] if has_bias else None]
        xg, wg = xd.detach().requires_grad_(True), wd.detach().requires_grad_(True)
        bg = bias.to(cuda).requires_grad_(True) if has_bias else None
        dwconv.depthwise_conv_tokens(xg, wg, bg, D, H, W).backward(dyd)
        return [xg.grad, wg.grad, bg.grad if has_bias else None]

    spy.calls.clear()
    dx, dw, db = run()
    assert [q for q, _, _ in spy.calls] == ["vivim_dwconv_wgrad_det_workspace_bytes"]
    r = {"dweight": fb.elem_ratio(dw, ref["dw"], bound["dw"])}
    if dx is not None:
        r["dx"] = fb.elem_ratio(dx, ref["dx"], bound["dx"])
    if has_bias:
        r["dbias"] = fb.elem_ratio(db, ref["db"], bound["db"])
    print(f"{(B, C, D, H, W)} {fb.name(dtype)} k3={k3} bias={has_bias}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items())
          + " (err / bound)")
    for k, v in r.items():
        fb.log_ratio(f"dwconv det {'3d' if k3 else '2d'} {k}", torch.float32 if k in ("dweight", "dbias") else dtype, (B, C, D, H, W), v)
    assert all(v <= 1.0 for v in r.values()), r
    _same_bits(spy, run, spy.calls[0][2], ["dx", "dweight", "dbias"])
