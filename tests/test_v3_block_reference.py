"""CPU: pins the float64 v3 block reference of tests/v3_block_cases.py, which test_gpu_v3_block.py measures every path against,
to oracle/ref_torch.py:mamba_v3_forward_ref (itself pinned to the reference module's fixtures by test_oracle.py) -- at the
tolerances test_oracle.py::test_v3_module_matches_reference uses for the same goldens: the two differ by fp32 round-off only.
Also the map references and block_errors themselves, on cases small enough to check by hand."""
import pytest
import torch

import v3_block_cases as vc
from conftest import golden_names, load_golden, rel_err
from oracle import ref_torch


def _golden(name):
    g = load_golden(name)
    params = {k[4:].replace("__", "."): v for k, v in g.items() if k.startswith("sd__")}
    return g, params, g["meta"][4]


@pytest.mark.parametrize("name", golden_names("module_"))
def test_fp64_forward_matches_ref_torch_and_golden(name):
    g, params, nf = _golden(name)
    with torch.no_grad():
        y64 = vc.v3_forward64(g["x"].double(), {k: v.double() for k, v in params.items()}, nf)
        y32 = ref_torch.mamba_v3_forward_ref(g["x"], params, nf)
    assert y64.dtype == torch.float64
    assert rel_err(y32, y64) < 1e-5
    assert rel_err(g["y"], y64) < 1e-5
    assert vc.token_error(y32, y64) < 1e-4          # and token by token: no token of the fp32 restatement is elsewhere


@pytest.mark.parametrize("name", ["module_nf5", "module_n64_e4_nf8"])
def test_fp64_gradients_match_ref_torch_and_golden(name):
    g, params, nf = _golden(name)
    ref = vc.v3_reference(g["x"], params, nf, dout=g["dout"])
    p32 = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    x32 = g["x"].clone().requires_grad_(True)
    ref_torch.mamba_v3_forward_ref(x32, p32, nf).backward(g["dout"])
    assert set(ref["grads"]) == set(params)
    assert rel_err(x32.grad, ref["dx"]) < 1e-4
    assert rel_err(g["dx"], ref["dx"]) < 1e-4
    for k in params:
        assert ref["grads"][k].dtype == torch.float64
        assert rel_err(p32[k].grad, ref["grads"][k]) < 2e-4, k
        assert rel_err(g["grad__" + k.replace(".", "__")], ref["grads"][k]) < 2e-4, k


def test_default_loss_is_mean_square():
    g, params, nf = _golden("module_nf3")
    y = vc.v3_reference(g["x"], params, nf)["y"]
    a = vc.v3_reference(g["x"], params, nf)
    b = vc.v3_reference(g["x"], params, nf, dout=2 * y / y.numel())
    assert rel_err(a["dx"], b["dx"]) < 1e-12 and all(rel_err(a["grads"][k], b["grads"][k]) < 1e-12 for k in params)


def test_map_references_by_hand():
    nf, hw = 3, 4
    x = torch.arange(nf * hw, dtype=torch.float32)                              # token t*hw+p holds t*hw+p
    a, b, c = vc.map_stack(x, nf)
    assert a.dtype == torch.float64 and a.tolist() == list(range(12)) and b.tolist() == list(range(11, -1, -1))
    assert c.tolist() == [0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7, 11]                 # position p*nf+t holds token t*hw+p
    for t in range(nf):
        for p in range(hw):
            assert c[p * nf + t] == x[t * hw + p]
    back = vc.map_unstack(a, b, c, nf)
    assert all(torch.equal(t, x.double()) for t in back)
    y = torch.randn(2, 3, 5 * 7)
    assert torch.equal(vc.deinterleave(vc.interleave(y, 5), 5), y)
    assert torch.equal(vc.interleave(y, 1), y) and torch.equal(vc.interleave(y, 35), y)


def test_block_errors_sees_one_misplaced_token():
    """Two tokens of y swapped: the per-token figure is of order 1 where the whole-tensor norm moves by a few per cent; a
    parameter gradient of one direction scaled by 1.5 shows as 0.5 on that tensor alone."""
    gen = torch.Generator().manual_seed(0)
    ref = {"y": torch.randn(2, 600, 8, generator=gen).double(), "dx": torch.randn(2, 600, 8, generator=gen).double(),
           "grads": {"D": torch.randn(16, generator=gen).double(), "D_b": torch.randn(16, generator=gen).double()}}
    got = {"y": ref["y"].clone(), "dx": ref["dx"].half(), "grads": {"D": ref["grads"]["D"].clone(), "D_b": ref["grads"]["D_b"] * 1.5}}
    got["y"][1, [300, 301]] = got["y"][1, [301, 300]]
    e = vc.block_errors(got, ref)
    assert set(e) == {"y", "dx", "grad:D", "grad:D_b"}
    assert e["y"] > 0.5 and rel_err(got["y"], ref["y"]) < 0.1
    assert 0 < e["dx"] < 2.0 ** -11 and e["grad:D"] == 0 and abs(e["grad:D_b"] - 0.5) < 1e-12
