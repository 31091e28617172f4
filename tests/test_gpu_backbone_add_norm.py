"""mamba_block(fused_backbone_add_norm=True): the one-stage model of tests/test_gpu_backbone_layernorm.py (hidden 64, 1 head,
sr_ratio 2, 2 blocks, 16 x 16 tokens, batch 3) with every residual add fused with the LayerNorm that reads the sum, against the
stock stage with the same weights -- which sites take which op, the dtypes under autocast, and accuracy judged against an fp64 copy
of the stock stage with that file's criterion: for the output and every parameter gradient
    err(fused) <= 2 * err(stock) + 2e-6      norm-wise
in fp32, under bf16 autocast, and in training mode with drop-path rate 0.5 (the fp64 stage replays the factors the run drew)."""
import copy
import functools
import os

import pytest
import torch
import torch.nn as nn

import conftest
from conftest import rel_err

pytestmark = pytest.mark.gpu


def _model(backbone, **kw):
    from vivim_amd.vivim import mamba_block
    return mamba_block(backbone, 3, depths=[0], dims=[64], **kw)     # depth 0: the Mamba stage is empty


@functools.lru_cache(maxsize=None)
def _models():
    """(stock, fused, fp64 stock on the CPU, input): equal weights, no dropout, no stochastic depth."""
    from transformers import SegformerConfig, SegformerForSemanticSegmentation
    cfg = SegformerConfig(num_channels=3, num_encoder_blocks=1, depths=[2], sr_ratios=[2], hidden_sizes=[64], patch_sizes=[7],
                          strides=[4], num_attention_heads=[1], mlp_ratios=[4], decoder_hidden_size=64, num_labels=3,
                          hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, drop_path_rate=0.0)
    torch.manual_seed(51)
    backbone = SegformerForSemanticSegmentation(cfg)
    g = torch.Generator().manual_seed(52)
    with torch.no_grad():
        for m in backbone.modules():                    # norms away from weight 1 / bias 0
            if isinstance(m, nn.LayerNorm):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 0.3 + 1.0)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
    stock = _model(copy.deepcopy(backbone))
    fused = _model(copy.deepcopy(backbone), fused_backbone_add_norm=True)
    ref64 = _model(copy.deepcopy(backbone)).double()
    assert list(fused.state_dict()) == list(stock.state_dict())
    x = torch.randn(1, 3, 3, 64, 64, generator=g)       # 3 frames, stride 4: 16 x 16 tokens
    return stock.cuda(), fused.cuda(), ref64, x


def _blocks(model):
    return list(model.downsample_layers.block[0])


def _fwd_bwd(model, x, autocast):
    for p in model.parameters():
        p.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast and x.is_cuda):
        out, = model(x)
    out.square().mean().backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return out.detach(), grads


@functools.lru_cache(maxsize=None)
def _reference():
    _, _, ref64, x = _models()
    return _fwd_bwd(ref64, x.double(), False)


def _trace(model, monkeypatch):
    """-> (calls, norms): every call of the three ops as (op, residual dtype, branch dtype, output dtypes), and the name of every
    LayerNorm module that was CALLED (a norm the fused route reads the Parameters of is not)."""
    from vivim_amd import layernorm as ln
    calls, norms = [], []
    real = {"add_layer_norm_tm": ln.add_layer_norm_tm, "add_tm": ln.add_tm, "layer_norm_tm": ln.layer_norm_tm}

    def wrap(op):
        def f(a, b, *rest, **kw):
            out = real[op](a, b, *rest, **kw)
            outs = out if isinstance(out, tuple) else (out,)
            calls.append((op, a.dtype, getattr(b, "dtype", None), tuple(t.dtype for t in outs)))
            return out
        return f
    for op in real:
        monkeypatch.setattr(ln, op, wrap(op))
    monkeypatch.setattr(ln, "tm_add_worthwhile", lambda res: True)    # 768 rows: whatever the measured threshold says
    for name, m in model.named_modules():
        if isinstance(m, nn.LayerNorm):
            m.register_forward_pre_hook(lambda mod, inp, name=name: norms.append(name))
    return calls, norms


def _short(names):
    return sorted(n.split("downsample_layers.")[-1] for n in names)


def _norm_names(model):
    """The names above in the installed transformers' spelling: the patch norm, the first block's first norm, the two
    sequence-reduction norms -- what stays a module call -- and the other three."""
    every = _short(n for n, m in model.named_modules() if isinstance(m, nn.LayerNorm) and "downsample_layers.layer_norm" not in n)
    assert len(every) == 7, every
    fused_away = [n for n in every if n.startswith("block.0.") and n.rsplit(".", 1)[-1] in
                  ("layernorm_after", "layer_norm_2") or n.startswith("block.0.1.") and n.rsplit(".", 1)[-1] in
                  ("layernorm_before", "layer_norm_1")]
    assert len(fused_away) == 3, fused_away
    return sorted(set(every) - set(fused_away)), every


def test_which_site_takes_which_op(cuda, monkeypatch):
    stock, fused, _, x = _models()
    monkeypatch.delenv("VIVIM_NO_FUSED_LAYERNORM", raising=False)
    fused, stock = copy.deepcopy(fused), copy.deepcopy(stock)             # the hooks stay on these copies
    calls, norms = _trace(fused, monkeypatch)
    kept, every = _norm_names(fused)
    _fwd_bwd(fused, x.to(cuda), False)
    # 2 * depth adds: 2 * depth - 1 with a norm, the stage's last alone; ATen norms the stage's first, the patch embedding's and
    # the sequence reductions' only
    assert [c[0] for c in calls] == ["add_layer_norm_tm"] * 3 + ["add_tm"], calls
    assert all(c[1:] == (torch.float32, torch.float32, (torch.float32,) * len(c[3])) for c in calls)
    assert _short(norms) == kept
    calls.clear(), norms.clear()
    monkeypatch.setenv("VIVIM_NO_FUSED_LAYERNORM", "1")                  # the stock call sequence again
    out_env, grads_env = _fwd_bwd(fused, x.to(cuda), False)
    assert not calls and _short(norms) == every
    monkeypatch.delenv("VIVIM_NO_FUSED_LAYERNORM")
    _, stock_norms = _trace(stock, monkeypatch)
    out_stock, grads_stock = _fwd_bwd(stock, x.to(cuda), False)
    assert not calls and _short(stock_norms) == every
    assert torch.equal(out_env, out_stock) and set(grads_env) == set(grads_stock)


def test_output_dtypes_under_autocast(cuda, monkeypatch):
    _, fused, _, x = _models()
    monkeypatch.delenv("VIVIM_NO_FUSED_LAYERNORM", raising=False)
    fused = copy.deepcopy(fused)
    calls, norms = _trace(fused, monkeypatch)
    out, _ = _fwd_bwd(fused, x.to(cuda), True)
    assert [c[0] for c in calls] == ["add_layer_norm_tm"] * 3 + ["add_tm"], calls
    for op, res_dtype, branch_dtype, outs in calls:
        # the stream stays fp32, the branch arrives in the autocast dtype and y leaves in it (what the norm's consumers cast to)
        assert res_dtype == torch.float32 and branch_dtype == torch.bfloat16
        assert outs == ((torch.float32, torch.bfloat16) if op == "add_layer_norm_tm" else (torch.float32,))
    assert out.dtype == torch.float32


def _compare(tag, autocast, want, stock_run, fused_run):
    (want_out, want_grads), (out_a, grads_a), (out_b, grads_b) = want, stock_run, fused_run
    assert set(grads_a) == set(grads_b) == set(want_grads)
    rows = [("out", rel_err(out_a, want_out), rel_err(out_b, want_out))]
    for n in sorted(want_grads):
        w = want_grads[n]
        if n.endswith("k_proj.bias") or n.endswith("key.bias"):
            # softmax does not see a shift of every key: this gradient is 0 in exact arithmetic, so its error is measured on the
            # scale of the weight's gradient (tests/test_gpu_backbone_layernorm.py)
            scale = want_grads[n[:-4] + "weight"].norm()
            if scale == 0:                               # every sample's attention branch of this block was dropped
                assert not grads_a[n].any() and not grads_b[n].any()
                continue
            assert w.norm() < 1e-12 * scale
            rows.append((n, float((grads_a[n].double().cpu() - w).norm() / scale), float((grads_b[n].double().cpu() - w).norm() / scale)))
        else:
            rows.append((n, rel_err(grads_a[n], w), rel_err(grads_b[n], w)))
    try:
        os.makedirs(os.path.dirname(conftest._PARITY_LOG), exist_ok=True)
        with open(conftest._PARITY_LOG, "a") as f:
            for n, ea, eb in rows:
                f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\tbackbone_add_norm {tag} {n}\t"
                        f"{'bf16 autocast' if autocast else 'float32'}\tstock_rel_err={ea:.3e}\tfused_rel_err={eb:.3e}\n")
    except OSError:
        pass
    for n, ea, eb in rows:
        print(f"{tag} {n}: stock {ea:.3e} fused {eb:.3e}")
    bad = [(n, ea, eb) for n, ea, eb in rows if not eb <= 2 * ea + 2e-6]
    assert not bad, bad


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16_autocast"])
def test_accuracy_against_the_fp64_stock_stage(autocast, cuda, monkeypatch):
    stock, fused, _, x = _models()
    monkeypatch.delenv("VIVIM_NO_FUSED_LAYERNORM", raising=False)
    calls, _ = _trace(copy.deepcopy(fused), monkeypatch)
    stock_run = _fwd_bwd(stock, x.to(cuda), autocast)
    assert not calls
    fused_run = _fwd_bwd(fused, x.to(cuda), autocast)
    assert len(calls) == 4
    _compare("eval", autocast, _reference(), stock_run, fused_run)


class _Replay(nn.Module):
    """Stochastic depth with the factors of an earlier run, one (batch,) vector per call, in call order."""

    def __init__(self, factors):
        super().__init__()
        self.factors = factors

    def forward(self, x):
        s = self.factors.pop(0).to(x.device, x.dtype)
        return x * s.view((-1,) + (1,) * (x.dim() - 1))


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16_autocast"])
def test_training_mode_with_drop_path(autocast, cuda, monkeypatch):
    """Rate 0.5 on both blocks: the factors DropPath.sample_scale returned are recorded, and the stock stage on the GPU and its fp64
    copy replay them (the same four calls in the same order)."""
    from vivim_amd.vivim import DropPath
    stock, fused, ref64, x = _models()
    monkeypatch.delenv("VIVIM_NO_FUSED_LAYERNORM", raising=False)
    stock, fused, ref64 = copy.deepcopy(stock).train(), copy.deepcopy(fused).train(), copy.deepcopy(ref64).train()
    for blk in _blocks(fused):
        blk.drop_path = DropPath(0.5)
    drawn = []
    real = DropPath.sample_scale
    monkeypatch.setattr(DropPath, "sample_scale", lambda self, t: (drawn.append(real(self, t)), drawn[-1])[1])
    calls, _ = _trace(fused, monkeypatch)
    torch.manual_seed(61)
    fused_run = _fwd_bwd(fused, x.to(cuda), autocast)
    assert [c[0] for c in calls] == ["add_layer_norm_tm"] * 3 + ["add_tm"] and len(drawn) == 4
    factors = [d.detach().cpu() for d in drawn]
    flat = torch.cat(factors)
    assert all(f.shape == (3,) and f.dtype == torch.float32 for f in factors) and bool(((flat == 0) | (flat == 2)).all())
    assert bool((flat == 0).any()) and bool((flat == 2).any())           # a dropped and a kept sample: both paths of the kernels
    runs = []
    for model, inp in ((stock, x.to(cuda)), (ref64, x.double())):
        replay = _Replay(list(factors))
        for blk in _blocks(model):
            blk.drop_path = replay
        runs.append(_fwd_bwd(model, inp, autocast))
        assert not replay.factors
    _compare("drop_path", autocast, runs[1], runs[0], fused_run)


def test_runs_and_matches_under_deterministic_algorithms(cuda, monkeypatch):
    stock, fused, _, x = _models()
    monkeypatch.delenv("VIVIM_NO_FUSED_LAYERNORM", raising=False)
    fused = copy.deepcopy(fused)
    calls, _ = _trace(fused, monkeypatch)
    stock_run = _fwd_bwd(stock, x.to(cuda), False)
    torch.use_deterministic_algorithms(True)
    try:
        first = _fwd_bwd(fused, x.to(cuda), False)
        second = _fwd_bwd(fused, x.to(cuda), False)
    finally:
        torch.use_deterministic_algorithms(False)
    assert [c[0] for c in calls] == (["add_layer_norm_tm"] * 3 + ["add_tm"]) * 2       # no atomics: the flag does not turn them away
    assert torch.equal(first[0], second[0]) and all(torch.equal(first[1][n], second[1][n]) for n in first[1])
    _compare("deterministic", False, _reference(), stock_run, first)
