"""What tests/test_abi_head_concat.py (CPU) and tests/test_gpu_head_concat.py (GPU) share: the shapes, the inputs, the fp64 reference
with its bounds, and the kernels' arithmetic restated in torch fp32 (restate32).

Reference.  M_h (OH x H_s), M_w are test_gpu_upsample.tap_matrix's per-axis matrices (the definition in fp32, placed in fp64);
k = keep * float32(1 / (1 - p)) placed in fp64 (1 where a map has no mask); per map
    want   = k (.) (M_h x M_w^T)                      x already rounded to the I/O dtype
    want_b = M_h^T (k (.) g_s) M_w                    g_s: the map's channel block of the output gradient
    S      = |M_h|^T (k (.) |g_s|) |M_w|,   G = (M_h > 0)^T (k (.) |g_s|) (M_w > 0)
Bounds, elementwise, u = 2^-23, rho = one unit in the last place of the I/O type (test_gpu_upsample.RHO), n_s = max(H_s, W_s),
T_s = 4 ceil(OH / H_s) ceil(OW / W_s):
    forward   |y - want|      <= (8 + 4 n_s) u max|x_s| scale_s + u |want| + rho |want| + tiny
                                 test_gpu_upsample's bound on v, carried through the product; the product's own rounding; the
                                 output rounding
    backward  |dx_s - want_b| <= (T_s + 6) u S + 4 n_s u G + rho |want_b| + tiny
                                 test_gpu_upsample's bound with one more rounding per term (dy * scale)
    a map of the output's own size: (u + rho) |want| + tiny, (u + rho) |want_b| + tiny: one product, one rounding
`tiny` corrects the derivation where rho |.| does not describe the output rounding: below the I/O type's smallest normal number
the spacing is fixed, and rounding to it errs by up to half of it whatever the value -- 2^-25 for fp16, 2^-134 for bf16, 2^-150 for
fp32.  With N(0, 1) inputs an fp16 result below 2^-14 is met about once in 10^4 elements; nothing else in the bounds covers it for
an equal-size map, where the other terms are relative as well.  It is a property of the number format, not a measured allowance."""
import functools
import math

import torch

from conftest import DT
from test_gpu_upsample import RHO, U, tap_matrix

# name: (N, [(C_s, H_s, W_s) ...] in concat order, (OH, OW))
SHAPES = {
    "ratios": (2, [(16, 1, 1), (16, 2, 2), (16, 4, 4), (16, 8, 8)], (8, 8)),     # the head's 8 / 4 / 2 / 1 ratios, an equal-size map
    "odd_c": (1, [(6, 3, 2), (13, 2, 3), (8, 7, 5)], (7, 5)),                    # counts and offsets that defeat the vector path
    "one_map": (2, [(8, 3, 3)], (5, 9)),
    "c768": (1, [(768, 1, 1), (768, 2, 2), (768, 4, 4), (768, 8, 8)], (8, 8)),   # bf16 only: the vector path at the real channel count
    "wide": (1, [(8, 4, 70), (8, 16, 300)], (16, 300)),                         # rows longer than one workgroup's piece
}
MASKS = ("none", "some", "all", "zero")      # masks on no map / every other map / every map / every map, map 0's all zero
P = 0.15
TINY = {torch.float32: 2.0 ** -150, torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134}
GRID = ([(name, dt, masks) for name in ("ratios", "odd_c", "one_map", "wide") for dt in ("fp32", "fp16", "bf16") for masks in MASKS]
        + [("c768", "bf16", masks) for masks in ("none", "some", "zero")])


def scale32(p):
    """float32(1 / (1 - p)) as a Python float: the factor the kernels multiply by."""
    return float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))


def masked(masks, s):
    return masks in ("all", "zero") or (masks == "some" and s % 2 == 0)


@functools.lru_cache(maxsize=None)
def case(name, dt, masks):
    """Inputs (rounded to the dtype) and fp64 references of one case, computed once and shared; nobody writes to them.
    maps[s] (N, C_s, H_s, W_s) and go (N, sum C_s, OH, OW) are contiguous CPU tensors; keep[s] is (N, OH, OW, C_s) uint8 or None."""
    N, shapes, (OH, OW) = SHAPES[name]
    dtype = DT[dt]
    g = torch.Generator().manual_seed(sum(map(ord, name + masks)))
    maps = [torch.randn(N, C, H, W, generator=g).to(dtype) for C, H, W in shapes]
    go = torch.randn(N, sum(C for C, _, _ in shapes), OH, OW, generator=g).to(dtype)
    keep, p = [], []
    for s, (C, H, W) in enumerate(shapes):
        on = masked(masks, s)
        k = (torch.rand(N, OH, OW, C, generator=g) >= P).to(torch.uint8) if on else None
        if on and masks == "zero" and s == 0:
            k.zero_()
        keep.append(k)
        p.append(P if on else None)
    refs, off = [], 0
    for s, (C, H, W) in enumerate(shapes):
        scale = scale32(P) if p[s] is not None else 1.0
        k64 = keep[s].permute(0, 3, 1, 2).double() * scale if keep[s] is not None else torch.ones(N, C, OH, OW, dtype=torch.float64)
        Mh, Mw = tap_matrix(H, OH), tap_matrix(W, OW)
        x64, g64 = maps[s].double(), go[:, off:off + C].double()
        want = k64 * torch.einsum("oh,nchw,pw->ncop", Mh, x64, Mw)
        want_b = torch.einsum("oh,ncop,pw->nchw", Mh, k64 * g64, Mw)
        S = torch.einsum("oh,ncop,pw->nchw", Mh.abs(), k64 * g64.abs(), Mw.abs())
        G = torch.einsum("oh,ncop,pw->nchw", (Mh > 0).double(), k64 * g64.abs(), (Mw > 0).double())
        n, T = max(H, W), 4 * math.ceil(OH / H) * math.ceil(OW / W)
        rho, tiny = RHO[dtype], TINY[dtype]
        if (H, W) == (OH, OW):
            fwd_bound, bwd_bound = (U + rho) * want.abs() + tiny, (U + rho) * want_b.abs() + tiny
        else:
            fwd_bound = (8 + 4 * n) * U * float(x64.abs().max()) * scale + U * want.abs() + rho * want.abs() + tiny
            bwd_bound = (T + 6) * U * S + 4 * n * U * G + rho * want_b.abs() + tiny
        refs.append(dict(want=want, want_b=want_b, S=S, T=T, k64=k64, fwd_bound=fwd_bound, bwd_bound=bwd_bound, off=off, scale=scale))
        off += C
    return dict(maps=maps, go=go, keep=keep, p=p, refs=refs, size=(OH, OW), dtype=dtype)


def worst(err, bound):
    """max err / bound, elementwise (a zero bound with a zero error counts as 0)."""
    return float(torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())


def within(err, bound, what):
    bad = err > bound
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, worst "
                                 f"{worst(err, bound):.3e} x, first at {bad.nonzero()[0].tolist()}")


def check(c, y, dxs, what):
    """Every map slice of y and every dx against the case's bounds -> (worst forward, worst backward) error as a share of the bound."""
    wf = wb = 0.0
    for s, r in enumerate(c["refs"]):
        C = c["maps"][s].shape[1]
        ey = (y[:, r["off"]:r["off"] + C].detach().double().cpu() - r["want"]).abs()
        ed = (dxs[s].detach().double().cpu() - r["want_b"]).abs()
        within(ey, r["fwd_bound"], f"{what}: y of map {s}")
        within(ed, r["bwd_bound"], f"{what}: dx of map {s}")
        wf, wb = max(wf, worst(ey, r["fwd_bound"])), max(wb, worst(ed, r["bwd_bound"]))
    return wf, wb


# ---- the kernels' arithmetic in torch fp32

def taps32(n_in, n_out):
    """up_tap for every output index of one axis, in fp32: (i0, i1, l0, l1).  src is the kernels' fused r * (o + 0.5) - 0.5: formed
    in fp64, where the product of two fp32 numbers is exact, and rounded to fp32."""
    r = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    o = torch.arange(n_out, dtype=torch.float32)
    src = torch.clamp((r.double() * (o.double() + 0.5) - 0.5).float(), min=0.0)
    i0 = src.to(torch.int64).clamp_max(n_in - 1)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    l1 = src - i0.to(torch.float32)
    return i0, i1, 1.0 - l1, l1


def _weights32(n_in, n_out):
    """(n_out, n_in) fp32: up_weight(tap(o), i)."""
    i0, i1, l0, l1 = taps32(n_in, n_out)
    cols = torch.arange(n_in)[None, :]
    return torch.where(i0[:, None] == cols, l0[:, None], torch.zeros(())) + torch.where(i1[:, None] == cols, l1[:, None], torch.zeros(()))


def restate32(maps, go, keep, scales, size, dtype):
    """head_concat.hip in torch fp32 on the CPU: the forward's expression per element, the select, one rounding; the backward's
    two nested ascending sums (a row's terms over ow first, then the rows over oh), the select on dy, one rounding.
    -> (y (N, sum C, OH, OW), [dx_s])."""
    OH, OW = size
    ys, dxs, off = [], [], 0
    for x, k, scale in zip(maps, keep, scales):
        N, C, H, W = x.shape
        x32, g32 = x.float(), go[:, off:off + C].float()
        kept = k.permute(0, 3, 1, 2) != 0 if k is not None else torch.ones(N, C, OH, OW, dtype=torch.bool)
        sc = torch.tensor(scale, dtype=torch.float32)
        zero = torch.zeros((), dtype=torch.float32)
        gk = torch.where(kept, g32 * sc, zero)
        if (H, W) == (OH, OW):
            v, dx = x32, gk
        else:
            h0, h1, lh0, lh1 = taps32(H, OH)
            w0, w1, lw0, lw1 = taps32(W, OW)
            a, b = x32[:, :, h0][:, :, :, w0], x32[:, :, h0][:, :, :, w1]
            d, e = x32[:, :, h1][:, :, :, w0], x32[:, :, h1][:, :, :, w1]
            lh0, lh1 = lh0[None, None, :, None], lh1[None, None, :, None]
            v = lh0 * (lw0 * a + lw1 * b) + lh1 * (lw0 * d + lw1 * e)
            Wh, Ww = _weights32(H, OH), _weights32(W, OW)
            racc = torch.zeros(N, C, OH, W, dtype=torch.float32)
            for ow in range(OW):                                       # a term outside the window is + 0 * g: exact
                racc += Ww[ow][None, None, None, :] * gk[:, :, :, ow:ow + 1]
            dx = torch.zeros(N, C, H, W, dtype=torch.float32)
            for oh in range(OH):
                dx += Wh[oh][None, None, :, None] * racc[:, :, oh:oh + 1, :]
        ys.append(torch.where(kept, v * sc, zero).to(dtype))
        dxs.append(dx.to(dtype))
        off += C
    return torch.cat(ys, dim=1), dxs


# ---- the head inside Vivim: one small model, recorded masks, and the three routes (stock, new, fp64) on the same inputs
HEAD_DIMS, HEAD_SIZES = (64, 128, 320, 512), (16, 8, 4, 2)
# torch.manual_seed(HEAD_SEED) makes all four coins say yes, MIXED_SEED gives (yes, no, yes, yes).  The comparison against fp64 runs
# with all four: in train mode BatchNorm removes every per-channel constant, so the bias of a projection whose map has no dropout
# has a gradient of exactly zero (max|want| ~ 1e-15 in fp64, pure rounding noise in every route) and there is nothing to compare.
HEAD_SEED, MIXED_SEED = 6, 5
# 4 x the worst max|err| / max|want| of the fp32 head on the CPU (the stock composition there: ATen's fp32 arithmetic of the kernels'
# form) against the fp64 head, over the logits and every head parameter's gradient.  The figure depends on how the CPU's BLAS splits
# its sums: 1.66e-6 with 16 threads, 1.86e-6 with 4, 3.67e-6 with one (the logits each time); FLOOR is 4 x the largest, and
# tests/test_abi_head_concat.py::test_the_fp32_head_on_the_cpu_sets_the_floor prints the figure and asserts 4 x it <= FLOOR.
FLOOR = 1.5e-5


def build_head(device, seed=HEAD_SEED):
    """A Vivim on a one-block-per-stage SegFormer from a local config in train mode, BatchNorm affine parameters and projection biases
    randomised, feature_dropout and the decoder's dropout at p = 0; four random encoder states of 4 frames, an output gradient, the
    coins that torch.manual_seed(seed) gives decode (stage order) and one recorded mask per stage whose coin says yes."""
    from transformers import SegformerConfig, SegformerForSemanticSegmentation
    from vivim_amd.decode_head import _projections
    from vivim_amd.vivim import Vivim
    torch.manual_seed(41)
    cfg = SegformerConfig(num_channels=3, num_encoder_blocks=4, depths=[1, 1, 1, 1], sr_ratios=[8, 4, 2, 1],
                          hidden_sizes=list(HEAD_DIMS), patch_sizes=[7, 3, 3, 3], strides=[4, 2, 2, 2],
                          num_attention_heads=[1, 2, 5, 8], mlp_ratios=[4, 4, 4, 4], decoder_hidden_size=768, num_labels=150)
    model = Vivim(in_chans=3, out_chans=3, depths=[1, 1, 1, 1], backbone=SegformerForSemanticSegmentation(cfg), fused_head_concat=True)
    g = torch.Generator().manual_seed(42)
    bn = model.decoder.batch_norm
    with torch.no_grad():
        bn.weight.copy_(torch.randn(768, generator=g))
        bn.bias.copy_(torch.randn(768, generator=g))
        for proj in _projections(model.decoder):
            proj.bias.copy_(torch.randn(768, generator=g))
    model.feature_dropout.p = 0.0
    model.decoder.dropout.p = 0.0
    model = model.to(device).train()
    N, (OH, OW) = 4, (HEAD_SIZES[0], HEAD_SIZES[0])
    states = tuple(torch.randn(N, c, s, s, generator=g).to(device) for c, s in zip(HEAD_DIMS, HEAD_SIZES))
    go = torch.randn(N, 3, OH, OW, generator=g).to(device)
    torch.manual_seed(seed)
    coins = [torch.rand(1).item() > 0.5 for _ in HEAD_DIMS]
    assert coins == ([True] * 4 if seed == HEAD_SEED else [True, False, True, True]), coins
    masks = [(torch.rand(N, OH, OW, 768, generator=g) >= model.dropout_rate / 2).to(torch.uint8).to(device) if coin else None
             for coin in coins]
    return dict(model=model, states=states, go=go, coins=coins, masks=masks, p=model.dropout_rate / 2, seed=seed)


def to_device(v, device):
    """A tensor, or the tensors of a list / tuple, on `device`; anything else as it is."""
    if torch.is_tensor(v):
        return v.to(device)
    return type(v)(to_device(t, device) for t in v) if isinstance(v, (list, tuple)) else v


class replayed:
    """While active, head_concat.draw_keep and the stock route's F.dropout(p = dropout_rate / 2) calls apply the recorded masks of
    `h` (keep * float32 scale, in the dtype of what they multiply) instead of drawing; every other F.dropout call is torch's.
    `drawn` counts the masks each route asked for."""

    def __init__(self, h):
        self.h, self.drawn = h, {"draw_keep": 0, "F.dropout": 0}

    def __enter__(self):
        import torch.nn.functional as F
        from vivim_amd import head_concat
        h, scale = self.h, scale32(self.h["p"])
        self.saved = (head_concat.draw_keep, F.dropout)
        stock = [m for m in h["masks"] if m is not None]                # F.dropout is called in stage order,
        fused = stock[::-1]                                             # draw_keep in concat order

        def draw_keep(shape, p, device):
            assert p == h["p"]
            mask = fused[self.drawn["draw_keep"]]
            self.drawn["draw_keep"] += 1
            assert tuple(shape) == tuple(mask.shape)
            return mask

        def dropout(x, p=0.5, training=True, inplace=False):
            if not (training and p == h["p"]):
                return self.saved[1](x, p, training, inplace)
            mask = stock[self.drawn["F.dropout"]]
            self.drawn["F.dropout"] += 1
            return x * (mask.permute(0, 3, 1, 2).to(x.dtype) * scale)

        head_concat.draw_keep, F.dropout = draw_keep, dropout
        return self

    def __exit__(self, *exc):
        import torch.nn.functional as F
        from vivim_amd import head_concat
        head_concat.draw_keep, F.dropout = self.saved


def run_head(h, model, switch, autocast=None, double=False):
    """One forward + backward of model.decode on h's states with the recorded masks -> (logits, {parameter name: gradient}, the
    tensor linear_fuse was handed, the number of masks each route asked for)."""
    model.fused_head_concat = switch
    seen = []
    hook = model.decoder.linear_fuse.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
    cast = (lambda t: t.double()) if double else (lambda t: t)
    try:
        with replayed(h) as rep:
            torch.manual_seed(h["seed"])
            model.zero_grad(set_to_none=True)
            if autocast is not None:
                with torch.autocast("cuda", dtype=autocast):
                    logits = model.decode(tuple(cast(s) for s in h["states"]), 1, 4)
            else:
                logits = model.decode(tuple(cast(s) for s in h["states"]), 1, 4)
            logits.backward(cast(h["go"]).to(logits.dtype))
    finally:
        hook.remove()
        model.fused_head_concat = True
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return logits.detach(), grads, seen[0], dict(rep.drawn)


def head_errors(got, want):
    """{name: (max|got - want|, max|want|)} over the logits and the gradients."""
    (logits, grads), (wl, wg) = got, want
    assert set(grads) == set(wg) and len(wg) == 13          # 4 projections, linear_fuse, batch_norm, out
    out = {"logits": (float((logits.double() - wl).abs().max()), float(wl.abs().max()))}
    for n in wg:
        out[n] = (float((grads[n].double() - wg[n]).abs().max()), float(wg[n].abs().max()))
    return out
