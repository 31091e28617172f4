"""The lean forward (vivim_selective_scan_fwd_lean, selective_scan_cuda.fwd_lean): for every forward kernel family it gives the
bits of the full forward -- out_z (out without z) and the final state -- and those bits agree with the CPU oracle; the
public wrappers take it exactly when no backward can follow, without leaking state into later grad-enabled calls; it
allocates neither `x` nor `out`; and it writes inside its buffers (VIVIM_GUARD child).  The file runs on the poisoned
allocator (conftest): `out_z` and `last_state` must be written in full by the kernels."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, SCAN_CLOSE, check_close, rel_err
from oracle import cpu_oracle

pytestmark = pytest.mark.gpu

FWD_VARIANTS = {"auto": 0, "nsplit_k8": 1, "nsplit_k4": 2, "generic": 3, "channels": 5, "states": 6}


@pytest.fixture(scope="module")
def ss(cuda):
    import selective_scan_cuda
    return selective_scan_cuda


@pytest.fixture
def pin():
    """vivim_set_tuning(0, variant) for the duration of a test (the forward selector; the backward is not used here)."""
    from vivim_amd import _lib
    L = _lib.lib()
    prev = []

    def set_(fwd):
        prev.append(L.vivim_set_tuning(0, fwd))

    yield set_
    if prev:
        L.vivim_set_tuning(0, prev[0])


_CASES = {}


def _case(dev, dtype, batch, dim, N, L, G, has_z=True, has_D=True, has_bias=True, softplus=True, strided=False, const_bc=False):
    """Inputs of one problem and the oracle's forward for them, made once and shared by the variants (read-only)."""
    key = (dtype, batch, dim, N, L, G, has_z, has_D, has_bias, softplus, strided, const_bc)
    if key in _CASES:
        return _CASES[key]
    gen = torch.Generator().manual_seed(hash(key[1:6]) % 100003 + 7 * has_z)

    def act(*shape):
        t = torch.randn(*shape, generator=gen).to(dtype)
        if strided and len(shape) == 3:                  # (L, B*L, 1) strides: a (D, B, L) buffer viewed as (B, D, L)
            return t.transpose(0, 1).contiguous().to(dev).transpose(0, 1)
        return t.to(dev)

    if softplus:                                         # module initialisation, mamba_simple.py:99-117
        A = -torch.arange(1, N + 1, dtype=torch.float32).repeat(dim, 1)
        delta = 0.2 * torch.randn(batch, dim, L, generator=gen)
        dtv = torch.exp(torch.rand(dim, generator=gen) * 4.605 - 6.908)
        bias = dtv + torch.log(-torch.expm1(-dtv))
    else:                                                # delta itself is the step: positive (test_selective_scan.py:87)
        A = -0.5 * torch.rand(dim, N, generator=gen)
        delta = 0.5 * torch.rand(batch, dim, L, generator=gen)
        bias = 0.5 * torch.rand(dim, generator=gen)
    delta = delta.to(dtype)
    delta = delta.transpose(0, 1).contiguous().to(dev).transpose(0, 1) if strided else delta.to(dev)
    if const_bc:
        Bm, Cm = torch.randn(dim, N, generator=gen).to(dev), torch.randn(dim, N, generator=gen).to(dev)
    else:
        Bm, Cm = act(batch, G, N, L), act(batch, G, N, L)
    t = dict(u=act(batch, dim, L), delta=delta, A=A.to(dev), B=Bm, C=Cm,
             D=torch.randn(dim, generator=gen).to(dev) if has_D else None, z=act(batch, dim, L) if has_z else None,
             delta_bias=bias.to(dev) if has_bias else None, softplus=softplus, dtype=dtype)
    t["ref"] = cpu_oracle.selective_scan_fwd(t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["z"], t["delta_bias"], softplus)
    _CASES[key] = t
    return t


def _lean_equals_full(t, ss):
    args = (t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["z"], t["delta_bias"], t["softplus"])
    full = ss.fwd(*args)
    ws_full = ss.last_workspace_bytes["fwd"]
    lean, last = ss.fwd_lean(*args, return_last_state=True)
    assert ss.last_workspace_bytes["fwd"] == ws_full
    want = full[2] if t["z"] is not None else full[0]
    assert lean.shape == want.shape and lean.stride() == want.stride() and lean.dtype == want.dtype
    assert torch.equal(lean, want), "lean result differs from the full forward's"
    x = full[1]
    assert last.shape == x[:, :, -1, :].shape and last.is_contiguous() and last.dtype == torch.float32
    assert torch.equal(last, x[:, :, -1, :]), "last_state differs from the last checkpoint row"
    only = ss.fwd_lean(*args)
    assert len(only) == 1 and torch.equal(only[0], want)                     # last_state == NULL
    r_out, r_out_z, r_last = t["ref"]
    dt = t["dtype"]
    check_close("lean", lean, (r_out_z if t["z"] is not None else r_out).to(dt).float(), dt, SCAN_CLOSE, 1e-3)
    check_close("last_state", last, r_last, torch.float32, SCAN_CLOSE, 1e-3)


@pytest.mark.parametrize("has_z", [True, False], ids=["z", "noz"])
@pytest.mark.parametrize("fwd", list(FWD_VARIANTS))
@pytest.mark.parametrize("dtype,batch,dim,L,G", [(torch.bfloat16, 3, 128, 2048, 1), (torch.float32, 2, 64, 1288, 1),
                                                (torch.float16, 2, 256, 320, 2), (torch.bfloat16, 1, 192, 8, 1)])
def test_lean_families_dstate16(fwd, has_z, dtype, batch, dim, L, G, cuda, ss, pin):
    """Every forward variant at dstate 16: 32 token-axis segments in the channels and the states family (segment inflow),
    a ragged last tile, two groups, and one unsegmented tile whose last token is the first checkpoint."""
    pin(FWD_VARIANTS[fwd])
    _lean_equals_full(_case(cuda, dtype, batch, dim, 16, L, G, has_z=has_z), ss)


@pytest.mark.parametrize("fwd", ["auto", "nsplit_k8", "generic", "channels", "states"])
@pytest.mark.parametrize("dtype,batch,dim,L,G", [(torch.bfloat16, 1, 384, 4104, 3), (torch.float32, 2, 64, 1000, 1),
                                                (torch.float16, 2, 128, 72, 2)])
def test_lean_families_dstate64(fwd, dtype, batch, dim, L, G, cuda, ss, pin):
    pin(FWD_VARIANTS[fwd])
    _lean_equals_full(_case(cuda, dtype, batch, dim, 64, L, G), ss)


@pytest.mark.parametrize("dtype,batch,dim,N,L,G,const_bc", [(torch.float32, 3, 5, 16, 333, 1, False),
                                                           (torch.float16, 3, 8, 200, 333, 2, False),
                                                           (torch.float32, 2, 12, 16, 700, 1, True)])
def test_lean_generic_only_shapes(dtype, batch, dim, N, L, G, const_bc, cuda, ss):
    """Shapes only the generic kernel takes: five channels, 200 states in two groups, constant B / C."""
    _lean_equals_full(_case(cuda, dtype, batch, dim, N, L, G, const_bc=const_bc), ss)


@pytest.mark.parametrize("fwd", ["channels", "states"])
def test_lean_vivim_strides(fwd, cuda, ss, pin):
    """(L, B*L, 1)-strided u / delta / z, as mamba_simple.py:204-208 produces them: out_z inherits z's strides."""
    pin(FWD_VARIANTS[fwd])
    t = _case(cuda, torch.bfloat16, 3, 128, 16, 2048, 1, strided=True)
    assert t["u"].stride() == (2048, 3 * 2048, 1)
    _lean_equals_full(t, ss)


@pytest.mark.parametrize("opts", [dict(has_D=False, has_bias=False), dict(has_D=False), dict(has_bias=False), dict(softplus=False)],
                         ids=["noD_nobias", "noD", "nobias", "nosoftplus"])
def test_lean_optional_arguments(opts, cuda, ss):
    _lean_equals_full(_case(cuda, torch.float32, 2, 12, 16, 700, 1, **opts), ss)


# ---------------------------------------------------------------------------------------------------- wrappers

D_INNER, N_STATE, SEQ, BATCH, RANK, D_MODEL = 64, 16, 192, 2, 4, 32


def _leaf(gen, dev, *shape, scale=1.0, dtype=torch.float32):
    return (torch.randn(*shape, generator=gen) * scale).to(dev, dtype).requires_grad_(True)


def _wrapper_problem(name, dev, dtype):
    """-> (fn, list of leaf tensors, builder of the positional arguments from the leaves)."""
    from vivim_amd import selective_scan_interface as si
    gen = torch.Generator().manual_seed(5)
    d, n, r, L, b = D_INNER, N_STATE, RANK, SEQ, BATCH
    a_log = lambda c: torch.log(torch.arange(1, n + 1, dtype=torch.float32)).repeat(c, 1).to(dev).requires_grad_(True)
    if name == "selective_scan_fn":
        leaves = [_leaf(gen, dev, b, d, L, dtype=dtype), _leaf(gen, dev, b, d, L, scale=0.2, dtype=dtype), a_log(d),
                  _leaf(gen, dev, b, n, L, dtype=dtype), _leaf(gen, dev, b, n, L, dtype=dtype), _leaf(gen, dev, d),
                  _leaf(gen, dev, b, d, L, dtype=dtype), _leaf(gen, dev, d, scale=0.1)]
        return si.selective_scan_fn, leaves, lambda u, dl, al, B, C, D, z, bias: (u, dl, -torch.exp(al), B, C, D, z, bias, True)
    if name == "mamba_inner_fn_no_out_proj":
        leaves = [_leaf(gen, dev, b, 2 * d, L, dtype=dtype), _leaf(gen, dev, d, 1, 4, scale=0.3), _leaf(gen, dev, d, scale=0.1),
                  _leaf(gen, dev, r + 2 * n, d, scale=d ** -0.5), _leaf(gen, dev, d, r, scale=r ** -0.5), a_log(d),
                  _leaf(gen, dev, d), _leaf(gen, dev, d, scale=0.1)]
        return (si.mamba_inner_fn_no_out_proj, leaves,
                lambda xz, cw, cb, xp, dp, al, D, bias: (xz, cw, cb, xp, dp, -torch.exp(al), None, None, D, bias, None, None, True))
    if name == "mamba_inner_grouped_fn_no_out_proj":
        G = 3
        leaves = [_leaf(gen, dev, b, 2, G, d, L, dtype=dtype), _leaf(gen, dev, G * d, 4, scale=0.3), _leaf(gen, dev, G * d, scale=0.1),
                  _leaf(gen, dev, G, r + 2 * n, d, scale=d ** -0.5), _leaf(gen, dev, G, d, r, scale=r ** -0.5), a_log(G * d),
                  _leaf(gen, dev, G * d), _leaf(gen, dev, G * d, scale=0.1)]
        return (si.mamba_inner_grouped_fn_no_out_proj, leaves,
                lambda xz, cw, cb, xp, dp, al, D, bias: (xz, cw, cb, xp, dp, -torch.exp(al), D, bias, True))
    assert name == "bimamba_inner_fn"
    leaves = [_leaf(gen, dev, b, 2 * d, L, dtype=dtype), _leaf(gen, dev, d, 1, 4, scale=0.3), _leaf(gen, dev, d, scale=0.1),
              _leaf(gen, dev, r + 2 * n, d, scale=d ** -0.5), _leaf(gen, dev, d, r, scale=r ** -0.5),
              _leaf(gen, dev, D_MODEL, d, scale=d ** -0.5), _leaf(gen, dev, D_MODEL, scale=0.1), a_log(d), a_log(d),
              _leaf(gen, dev, d), _leaf(gen, dev, d, scale=0.1)]
    return (si.bimamba_inner_fn, leaves,
            lambda xz, cw, cb, xp, dp, ow, ob, al, alb, D, bias: (xz, cw, cb, xp, dp, ow, ob, -torch.exp(al), -torch.exp(alb),
                                                                   None, None, D, bias, None, None, True))


WRAPPERS = ["selective_scan_fn", "mamba_inner_fn_no_out_proj", "mamba_inner_grouped_fn_no_out_proj", "bimamba_inner_fn"]


@pytest.mark.parametrize("amp", [True, False], ids=["bf16_autocast", "fp32"])
@pytest.mark.parametrize("name", WRAPPERS)
def test_wrappers_take_the_lean_route_without_a_backward(name, amp, cuda, ss, monkeypatch):
    """no_grad / inference_mode / no argument requiring grad give the bits of the grad-enabled call (itself the same with
    the lean route switched off), call fwd_lean and never fwd; a grad-enabled call afterwards still takes the full route
    and backpropagates to the gradients of the first, untouched call."""
    dtype = torch.bfloat16 if amp else torch.float32
    fn, leaves, build = _wrapper_problem(name, cuda, dtype)
    calls = []
    real_fwd, real_lean = ss.fwd, ss.fwd_lean
    from vivim_amd import selective_scan_cuda as impl
    monkeypatch.setattr(impl, "fwd", lambda *a, **k: (calls.append("fwd"), real_fwd(*a, **k))[1])
    monkeypatch.setattr(impl, "fwd_lean", lambda *a, **k: (calls.append("lean"), real_lean(*a, **k))[1])

    def run(grad):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            y = fn(*build(*leaves))
        if not grad:
            return y, None
        gen = torch.Generator().manual_seed(1)
        for t in leaves:
            t.grad = None
        (y.float() * torch.randn(y.shape, generator=gen).to(cuda)).sum().backward()
        return y.detach(), [t.grad.clone() for t in leaves]

    monkeypatch.setenv("VIVIM_NO_LEAN_FWD", "1")
    y_ref, g_ref = run(True)                               # before any lean call: the untouched state
    with torch.no_grad():
        y_off, _ = run(False)
    assert calls == ["fwd", "fwd"] and torch.equal(y_off, y_ref)
    monkeypatch.delenv("VIVIM_NO_LEAN_FWD")
    del calls[:]
    y_on, g_on = run(True)
    assert calls == ["fwd"] and torch.equal(y_on, y_ref)
    del calls[:]
    with torch.no_grad():
        y_ng, _ = run(False)
    with torch.inference_mode():
        y_im, _ = run(False)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        y_det = fn(*build(*[t.detach() for t in leaves]))  # grad mode on, nothing requires grad
    assert calls == ["lean"] * 3
    for y in (y_ng, y_im, y_det):
        assert not y.requires_grad and y.dtype == y_ref.dtype and torch.equal(y, y_ref)
    del calls[:]
    y_after, g_after = run(True)
    assert calls == ["fwd"] and torch.equal(y_after, y_ref)
    # The backward adds its reductions with float atomics, so two runs differ by the order of fp32 sums, and under bf16 by
    # at most one rounding of a bf16 gradient element (2^-8): norm-wise bounds from the formats, far below what a stale or
    # missing saved tensor would give (order 1).  The same bound holds between the two untouched runs.
    tol = 4e-3 if amp else 1e-4
    for a, b, c in zip(g_after, g_ref, g_on):
        assert torch.isfinite(a).all() and rel_err(a, b) < tol and rel_err(c, b) < tol


def test_selective_scan_fn_last_state_is_the_kernel_buffer(cuda, ss):
    from mamba_ssm.ops.selective_scan_interface import selective_scan_fn
    t = _case(cuda, torch.bfloat16, 3, 128, 16, 2048, 1)
    args = (t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["z"], t["delta_bias"], True)
    y, last = selective_scan_fn(*args, return_last_state=True)             # nothing requires grad: lean
    assert last.is_contiguous() and last.shape == (3, 128, 16) and last.dtype == torch.float32
    full = ss.fwd(*args)
    assert torch.equal(last, full[1][:, :, -1, :]) and torch.equal(y, full[2])
    u = t["u"].clone().requires_grad_(True)
    y2, last2 = selective_scan_fn(u, *args[1:], return_last_state=True)    # the autograd route: today's view of x
    assert y2.requires_grad and torch.equal(y2.detach(), y) and torch.equal(last2, last)


def test_lean_allocates_neither_x_nor_out(cuda, ss):
    """Arithmetic on the allocator's peak: the full call holds out, x, out_z and the workspace, the lean call out_z, the
    49 KB last_state and the same workspace; 0.9 leaves room for the allocator's 512-byte rounding."""
    t = _case(cuda, torch.bfloat16, 3, 384, 16, 4096, 3)
    args = (t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["z"], t["delta_bias"], True)

    def peak(call):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res = call()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, res

    d_full, full = peak(lambda: ss.fwd(*args))
    x_bytes, out_bytes = full[1].nbytes, full[0].nbytes
    del full
    d_lean, lean = peak(lambda: ss.fwd_lean(*args, return_last_state=True))
    print(f"peak delta full {d_full} lean {d_lean} x {x_bytes} out {out_bytes}")
    assert d_full - d_lean >= 0.9 * (x_bytes + out_bytes), (d_full, d_lean, x_bytes, out_bytes)


CHILD = r"""
import torch
from vivim_amd import _lib
import selective_scan_cuda as ss
assert _lib.GUARD
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
n_calls = 0
for fwd_v in (0, 1, 3, 5, 6):
    _lib.lib().vivim_set_tuning(0, fwd_v)
    for (B, D, N, L, G, dt) in ((2, 24, 16, 333, 1, torch.float32), (1, 96, 16, 2100, 3, torch.bfloat16),
                                (1, 20, 64, 150, 2, torch.float16), (2, 8, 32, 17, 1, torch.float32)):
        mk = lambda *s: torch.randn(*s, generator=g).to(dev).to(dt)
        u, delta, z = mk(B, D, L), 0.3 * mk(B, D, L), mk(B, D, L)
        A = -(torch.rand(D, N, generator=g) + 0.1).to(dev)
        Bm, Cm = mk(B, G, N, L), mk(B, G, N, L)
        Dv, bias = torch.randn(D, generator=g).to(dev), torch.rand(D, generator=g).to(dev)
        for zz in (z, None):
            res = ss.fwd_lean(u, delta, A, Bm, Cm, Dv, zz, bias, True, True)
            _lib.check_guards("fwd_lean")
            assert all(torch.isfinite(t.float()).all() for t in res)
            n_calls += 1
_lib.lib().vivim_set_tuning(0, 0)
from mamba_ssm import Mamba
m = Mamba(d_model=32, bimamba_type="v3", nframes=3).to(dev)
xin = torch.randn(2, 3 * 64, 32, device=dev)
with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
    yy = m(xin)
_lib.check_guards("module, no grad")
assert torch.isfinite(yy.float()).all()
print("LEAN_GUARD_OK", n_calls)
"""


def test_lean_forward_under_guard(cuda):
    env = dict(os.environ, VIVIM_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("VIVIM_NO_LEAN_FWD", None)
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "LEAN_GUARD_OK 40" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
