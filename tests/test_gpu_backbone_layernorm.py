"""mamba_block(fast_backbone_layernorm=True): one SegFormer stage (hidden 64, 1 head, sr_ratio 2, 2 blocks, 16 x 16 tokens, batch 3)
with its LayerNorms swapped against the stock stage with the same weights -- which norm takes which kernel, the output dtypes
under autocast, and accuracy judged against an fp64 copy of the stock stage: for the output and every parameter gradient
    err(swapped) <= 2 * err(stock) + 2e-6      norm-wise
(2: the one extra 16-bit rounding where two low-precision gradients meet at layernorm_before's output, and the kernels' different
but equally ordered fp32 sums; 2e-6: the project's fp32 LayerNorm bound).  Measured on an MI355X: fp32 output 8.2e-8 stock and 1.3e-7
swapped, gradients 5e-8 .. 5e-7 with swapped / stock between 0.83 and 1.56; bf16 autocast output 2.824e-3 either way, gradients
5e-4 .. 7e-3 with swapped / stock between 0.87 and 1.11."""
import copy
import functools
import os

import pytest
import torch
import torch.nn as nn

import conftest
from conftest import rel_err

pytestmark = pytest.mark.gpu


class _Stage(nn.Module):
    def __init__(self, backbone):
        super().__init__()
        from vivim_amd.vivim import _Encoder
        self.enc = _Encoder(backbone)

    def forward(self, x):
        from vivim_amd.vivim import _run_block
        hs, height, width = self.enc.patch_embeddings[0](x)
        for blk in self.enc.block[0]:
            hs = _run_block(blk, hs, height, width)
        return hs


@functools.lru_cache(maxsize=None)
def _stages():
    """(stock, swapped, fp64 stock on the CPU, input): equal weights, no dropout, no stochastic depth."""
    from transformers import SegformerConfig, SegformerForSemanticSegmentation
    from vivim_amd.vivim import _swap_backbone_layernorm
    cfg = SegformerConfig(num_channels=3, num_encoder_blocks=1, depths=[2], sr_ratios=[2], hidden_sizes=[64], patch_sizes=[7],
                          strides=[4], num_attention_heads=[1], mlp_ratios=[4], decoder_hidden_size=64, num_labels=3,
                          hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, drop_path_rate=0.0)
    torch.manual_seed(51)
    stock = _Stage(SegformerForSemanticSegmentation(cfg))
    g = torch.Generator().manual_seed(52)
    with torch.no_grad():
        for m in stock.modules():                       # norms away from weight 1 / bias 0
            if isinstance(m, nn.LayerNorm):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 0.3 + 1.0)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
    ref64 = copy.deepcopy(stock).double()
    swapped = copy.deepcopy(stock)
    assert _swap_backbone_layernorm(swapped.enc) == 1 + 2 * 3
    x = torch.randn(3, 3, 64, 64, generator=g)          # stride 4: 16 x 16 tokens
    return stock.cuda(), swapped.cuda(), ref64, x


def _fwd_bwd(stage, x, autocast):
    for p in stage.parameters():
        p.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast and x.is_cuda):
        out = stage(x)
    out.square().mean().backward()                      # the residual stream: fp32 (fp64 for the reference) under autocast too
    grads = {n: p.grad.detach().clone() for n, p in stage.named_parameters() if p.grad is not None}
    return out.detach(), grads


@functools.lru_cache(maxsize=None)
def _reference():
    _, _, ref64, x = _stages()
    return _fwd_bwd(ref64, x.double(), False)


def _trace(stage, monkeypatch):
    """-> {norm's module name: ("cm" | "tm", its input's channel stride, input dtype, output dtype)}, filled in as `stage` runs:
    which of the library's two LayerNorm ops each swapped norm calls (a norm that stays on ATen leaves no entry)."""
    from vivim_amd import layernorm as ln
    from vivim_amd.vivim import _BackboneLayerNorm
    taken, current = {}, []
    real = {"cm": ln.layer_norm_cm, "tm": ln.layer_norm_tm}

    def wrap(kind):
        def op(x, *a, **k):
            y = real[kind](x, *a, **k)
            taken[current[-1]] = (kind, x.stride(-1), x.dtype, y.dtype)
            return y
        return op
    monkeypatch.setattr(ln, "layer_norm_cm", wrap("cm"))
    monkeypatch.setattr(ln, "layer_norm_tm", wrap("tm"))
    monkeypatch.setattr(ln, "worthwhile", lambda x: True)   # 768 tokens: below both families' break-even on host time
    monkeypatch.setattr(ln, "tm_worthwhile", lambda x: True)
    for name, m in stage.named_modules():
        if isinstance(m, _BackboneLayerNorm):
            m.register_forward_pre_hook(lambda mod, inp, name=name: current.append(name))
    return taken


PATCH = "enc.patch_embeddings.0.layer_norm"


def _is_block_norm(name):
    return name.rsplit(".", 1)[-1] in ("layernorm_before", "layernorm_after", "layer_norm_1", "layer_norm_2")


def _check_paths(taken):
    """The patch embedding's norm reads the channel-major view of its conv's output: layer_norm_cm.  before / after of the two
    blocks read token-major rows: layer_norm_tm.  The two sequence-reduction norms read `conv_out.reshape(B, C, -1).transpose(1, 2)`:
    channel-major when the conv writes (B, C, H, W) planes, rows when it answers its channels-last input with a channels-last
    output -- each takes the kernel for the layout it is handed, none ATen."""
    assert len(taken) == 7, sorted(taken)
    assert taken[PATCH][:2] == ("cm", 16 * 16)
    block = [n for n in taken if _is_block_norm(n)]
    assert len(block) == 4 and all(taken[n][:2] == ("tm", 1) for n in block)
    reduction = [n for n in taken if n != PATCH and n not in block]
    assert len(reduction) == 2 and all("attention" in n for n in reduction)
    for n in reduction:
        assert taken[n][0] == ("tm" if taken[n][1] == 1 else "cm"), (n, taken[n])


def test_which_norm_takes_which_kernel(cuda, monkeypatch):
    stock, swapped, _, x = _stages()
    monkeypatch.delenv("VIVIM_NO_FUSED_LAYERNORM", raising=False)
    swapped = copy.deepcopy(swapped)                        # the hooks stay on this copy
    taken = _trace(swapped, monkeypatch)
    assert swapped.state_dict().keys() == stock.state_dict().keys()
    _fwd_bwd(swapped, x.to(cuda), False)
    _check_paths(taken)
    assert all(t[2] == t[3] == torch.float32 for t in taken.values())
    taken.clear()
    _fwd_bwd(stock, x.to(cuda), False)
    assert not taken
    monkeypatch.setenv("VIVIM_NO_FUSED_LAYERNORM", "1")
    _fwd_bwd(swapped, x.to(cuda), False)
    assert not taken                                        # all of them on ATen


def test_output_dtypes_under_autocast(cuda, monkeypatch):
    _, swapped, _, x = _stages()
    monkeypatch.delenv("VIVIM_NO_FUSED_LAYERNORM", raising=False)
    swapped = copy.deepcopy(swapped)
    taken = _trace(swapped, monkeypatch)
    _fwd_bwd(swapped, x.to(cuda), True)
    _check_paths(taken)
    for name, (_, _, in_dtype, out_dtype) in taken.items():
        # the patch embedding writes the fp32 residual stream; every norm inside a block feeds Linears and Convs only
        assert out_dtype == (torch.float32 if name == PATCH else torch.bfloat16), (name, out_dtype)
        if _is_block_norm(name):
            assert in_dtype == torch.float32                # the residual stream, rounded once in the kernel


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16_autocast"])
def test_accuracy_against_the_fp64_stock_stage(autocast, cuda, monkeypatch):
    stock, swapped, _, x = _stages()
    monkeypatch.delenv("VIVIM_NO_FUSED_LAYERNORM", raising=False)
    swapped = copy.deepcopy(swapped)
    taken = _trace(swapped, monkeypatch)
    want_out, want_grads = _reference()
    out_a, grads_a = _fwd_bwd(stock, x.to(cuda), autocast)
    assert not taken
    out_b, grads_b = _fwd_bwd(swapped, x.to(cuda), autocast)
    _check_paths(taken)
    assert set(grads_a) == set(grads_b) == set(want_grads)
    rows = [("out", rel_err(out_a, want_out), rel_err(out_b, want_out))]
    for n in sorted(want_grads):
        want = want_grads[n]
        if n.endswith("k_proj.bias"):
            # softmax does not see a shift of every key, so this gradient is 0 in exact arithmetic (1e-20 in the fp64 run) and an
            # error relative to it is the ratio of two rounding residues: it is measured on the scale of k_proj.weight's gradient
            scale = want_grads[n[:-4] + "weight"].norm()
            assert want.norm() < 1e-12 * scale
            rows.append((n, float((grads_a[n].double().cpu() - want).norm() / scale),
                         float((grads_b[n].double().cpu() - want).norm() / scale)))
        else:
            rows.append((n, rel_err(grads_a[n], want), rel_err(grads_b[n], want)))
    try:
        os.makedirs(os.path.dirname(conftest._PARITY_LOG), exist_ok=True)
        with open(conftest._PARITY_LOG, "a") as f:
            for n, ea, eb in rows:
                f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\tbackbone_layernorm {n}\t"
                        f"{'bf16 autocast' if autocast else 'float32'}\tstock_rel_err={ea:.3e}\tswapped_rel_err={eb:.3e}\n")
    except OSError:
        pass
    for n, ea, eb in rows:
        print(f"{n}: stock {ea:.3e} swapped {eb:.3e}")
    bad = [(n, ea, eb) for n, ea, eb in rows if not eb <= 2 * ea + 2e-6]
    assert not bad, bad
