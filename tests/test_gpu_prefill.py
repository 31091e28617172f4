"""Mamba.forward(inference_params=...): the prefill (seqlen_offset == 0) fills the cache `step` advances -- conv_state with the
last d_conv pre-conv columns, ssm_state with the scan's final state -- and later calls are single-token steps
(mamba_simple.py:196-201, :311-353).  fp32 throughout; the bound is the one tests/test_gpu_update.py uses for the same
comparison of the stepped recurrence with the full-sequence path."""
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 2e-5
B, D_MODEL = 2, 32


def _module(dev, layer_idx=0, seed=3):
    from mamba_ssm import Mamba
    torch.manual_seed(seed)
    return Mamba(d_model=D_MODEL, d_state=16, d_conv=4, expand=2, bimamba_type="v3", layer_idx=layer_idx).to(dev)


def _full_sequence(m, x):
    """The forward-direction full-sequence path built from the module's parameters (in_proj -> fused inner op -> out_proj)."""
    from mamba_ssm.ops.selective_scan_interface import mamba_inner_fn
    b, L, _ = x.shape
    xz = (m.in_proj.weight @ x.reshape(b * L, -1).t()).view(2 * m.d_inner, b, L).transpose(0, 1)
    return mamba_inner_fn(xz, m.conv1d.weight, m.conv1d.bias, m.x_proj.weight, m.dt_proj.weight, m.out_proj.weight,
                          m.out_proj.bias, -torch.exp(m.A_log.float()), None, None, m.D.float(),
                          delta_bias=m.dt_proj.bias.float(), delta_softplus=True)


@pytest.mark.parametrize("prompt", [24, 2, 1])
def test_prefill_then_step_matches_full_sequence_and_stepping(prompt, cuda):
    """Prompts of 24 tokens, and of 2 and 1 (shorter than d_conv: conv_state is left-padded with zeros)."""
    from vivim_amd import InferenceParams
    m = _module(cuda)
    total = prompt + 3
    x = torch.randn(B, total, D_MODEL, device=cuda)
    with torch.no_grad():
        full = _full_sequence(m, x)
        ip = InferenceParams(max_seqlen=total, max_batch_size=B)
        outs = [m(x[:, :prompt], inference_params=ip)]
        assert outs[0].shape == (B, prompt, D_MODEL)
        conv_state, ssm_state = ip.key_value_memory_dict[0]
        # the states 24 (2, 1) `step` calls reach from a fresh cache
        cs, hs = m.allocate_inference_cache(B, total)
        for t in range(prompt):
            m.step(x[:, t:t + 1], cs, hs)
        assert rel_err(ssm_state, hs) < TOL and rel_err(conv_state, cs) < TOL
        for t in range(prompt, total):
            ip.seqlen_offset = t
            o = m(x[:, t:t + 1], inference_params=ip)
            assert o.shape == (B, 1, D_MODEL)
            outs.append(o)
        assert ip.key_value_memory_dict[0][0] is conv_state and ip.key_value_memory_dict[0][1] is ssm_state
    assert rel_err(torch.cat(outs, dim=1), full) < TOL


def test_prefill_uses_the_lean_forward_under_no_grad(cuda, monkeypatch):
    from vivim_amd import InferenceParams, selective_scan_cuda as impl
    calls = []
    real_fwd, real_lean = impl.fwd, impl.fwd_lean
    monkeypatch.setattr(impl, "fwd", lambda *a, **k: (calls.append("fwd"), real_fwd(*a, **k))[1])
    monkeypatch.setattr(impl, "fwd_lean", lambda *a, **k: (calls.append("lean"), real_lean(*a, **k))[1])
    m = _module(cuda)
    x = torch.randn(B, 24, D_MODEL, device=cuda)
    with torch.no_grad():
        m(x, inference_params=InferenceParams(24, B))
    assert calls == ["lean"]


def test_cache_keying(cuda):
    from mamba_ssm.utils.generation import InferenceParams
    m0, m1 = _module(cuda, 0), _module(cuda, 1, seed=4)
    x = torch.randn(B, 8, D_MODEL, device=cuda)
    ip = InferenceParams(max_seqlen=16, max_batch_size=B)
    with torch.no_grad():
        m0(x, inference_params=ip)
        ptrs = [t.data_ptr() for t in ip.key_value_memory_dict[0]]
        assert [t.shape for t in ip.key_value_memory_dict[0]] == [(B, 64, 4), (B, 64, 16)]
        m0(x, inference_params=ip)                                          # a second prefill reuses the same tensors
        assert [t.data_ptr() for t in ip.key_value_memory_dict[0]] == ptrs
        ip.seqlen_offset = 8
        m0(x[:, :1], inference_params=ip)
        assert [t.data_ptr() for t in ip.key_value_memory_dict[0]] == ptrs
        m1(x[:, :1], inference_params=ip)                                   # another layer gets its own (stepping from zeros)
        assert set(ip.key_value_memory_dict) == {0, 1}
        assert not set(t.data_ptr() for t in ip.key_value_memory_dict[1]) & set(ptrs)
        got = m0._get_states_from_cache(ip, B)
        assert [t.data_ptr() for t in got] == ptrs
        m0._get_states_from_cache(ip, B, initialize_states=True)
        assert all(float(t.abs().max()) == 0.0 for t in ip.key_value_memory_dict[0])

    class Duck:                                                             # any object with the two fields
        seqlen_offset = 0

        def __init__(self):
            self.key_value_memory_dict = {}

    with torch.no_grad():
        d = Duck()
        y = m0(x, inference_params=d)
        assert y.shape == x.shape and 0 in d.key_value_memory_dict
    with pytest.raises(AssertionError):
        _module(cuda, None)(x, inference_params=InferenceParams(16, B))


def test_prefill_backpropagates(cuda):
    from vivim_amd import InferenceParams
    m = _module(cuda)
    x = torch.randn(B, 24, D_MODEL, device=cuda, requires_grad=True)
    ip = InferenceParams(24, B)
    y = m(x, inference_params=ip)
    assert y.requires_grad
    y.square().mean().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
    for p in (m.in_proj.weight, m.conv1d.weight, m.x_proj.weight, m.dt_proj.weight, m.A_log, m.D, m.out_proj.weight):
        assert p.grad is not None and torch.isfinite(p.grad).all()
    with torch.no_grad():                                                   # the cache was filled on the way
        assert rel_err(ip.key_value_memory_dict[0][1], _states_by_stepping(m, x.detach())[1]) < TOL


def _states_by_stepping(m, x):
    cs, hs = m.allocate_inference_cache(x.shape[0], x.shape[1])
    for t in range(x.shape[1]):
        m.step(x[:, t:t + 1], cs, hs)
    return cs, hs
