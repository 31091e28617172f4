"""Inputs, fp64 reference, fp32 restatement and bounds of the structure loss, shared by tests/test_abi_structure_loss.py (CPU) and
tests/test_gpu_structure_loss.py (GPU): both run the same cases and hold them to the same bounds.

Reference: the reference's formula (final_multiclass_training.py:403-445, train_binary.py:57-67) written out below in fp64 on the CPU
from the same rounded inputs, the gradient by autograd.  `restate32` is the arithmetic of csrc/structure_loss.hip in torch fp32:
integer window counts from two 31-tap passes, the weight from one division, sigmoid(-x) for 1 - sigmoid(x), the four sums without a
subtraction, the gradient formula with the finalise kernel's three factors.

Bounds (those of tests/test_gpu_seg_loss.py, with the elementwise one in the err <= 2 * err(eager) + floor form):
    loss        |loss - loss64| <= 1e-5 * |loss64|
    dlogits     norm-wise < 1e-3 against fp64 (for 16-bit logits: against fp64 rounded to the dtype)
    16-bit      dlogits within one rounding of the fp32 value: |g16 - g32| <= u * |g32| * (1 + 2^-10) + 1e-5 * |g32| + tiny, g32 what the
                same code gives for the same logits widened to fp32, u = 2^-11 / 2^-8 (fp16 / bf16), 1e-5 for the two fp32 evaluations
                (their tiles, and so the last bits of their sums, differ; each holds the 1e-5 loss bound), tiny = 2^-25 (half of fp16's
                smallest subnormal; bf16 has fp32's range)
    elementwise |g32 - g64| <= 2 * |eager32 - g64| + FLOOR * max|g64|, eager32 the eager fp32 composition on the same inputs

FLOOR.  Not a property of the formula but of fp32: measured as the worst |restate32 - g64| / max|g64| over every case below (all
shapes, scales 1 / 8 / 30, every label content), which is 3.62e-7 (c8, fp16-rounded logits, scale 1;
test_abi_structure_loss.py prints it), times the margin of 4 and rounded up: 1.5e-6.  The eager composition's own worst figure over the same cases is printed next to it."""
import torch
import torch.nn.functional as F

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = {"fp32": F32, "bf16": BF16, "fp16": F16}
U_ROUND = {F16: 2.0 ** -11, BF16: 2.0 ** -8}
SCALES = (1.0, 8.0, 30.0)
FLOOR = 1.5e-6
WIN, HALO = 31, 15

# name -> (N, C, H, W), first_class, eps.  H, W below the window; exactly the window; odd and more than one tile down; the c5 fixture's
# shape; a whole number of tiles with 8 classes; three tiles across with halos over both tile edges.
SHAPES = {
    "binary": ((2, 1, 5, 7), 1, 1.0),
    "win31": ((1, 2, 31, 31), 0, 1e-6),
    "odd": ((2, 3, 33, 47), 0, 1e-6),
    "c5": ((1, 5, 40, 31), 0, 1e-6),
    "c8": ((3, 8, 64, 64), 0, 1e-6),
    "wide": ((1, 3, 20, 130), 0, 1e-6),
}
CONTENTS = ("mixed", "solid", "holes")


def make_case(name, dtype, scale, seed=0, content="mixed"):
    """-> logits (N, C, H, W) randn * scale rounded to `dtype`, targets (N, H, W) int64, on the CPU.  Labels: noise over a solid block
    (windows that are full, empty and in between).  "mixed": image 0 lacks its last class; "solid": image 0 is one class only;
    "holes": a fifth of the labels are values outside the classes (255, C + first_class, -1, 2^32 + 1)."""
    (N, C, H, W), first, _ = SHAPES[name]
    g = torch.Generator().manual_seed(seed * 1000 + N * 100 + C * 10 + H)
    logits = (torch.randn(N, C, H, W, generator=g) * scale).to(dtype)
    lo, hi = (0, 2) if C == 1 else (first, first + C)
    targets = torch.randint(lo, hi, (N, H, W), generator=g)
    targets[:, : H // 2, : max(W // 3, 1)] = hi - 1
    targets[0][targets[0] == hi - 1] = lo                       # image 0: the last class (binary: the foreground) is absent
    if content == "solid":
        targets[0] = first
    elif content == "holes":
        other = torch.tensor([255, hi, -1, 2 ** 32 + 1])[torch.randint(0, 4, (N, H, W), generator=g)]
        targets = torch.where(torch.rand(N, H, W, generator=g) < 0.2, other, targets)
    return logits, targets


def masks(targets, C, first):
    return targets.long()[:, None] == (torch.arange(C, device=targets.device) + first)[None, :, None, None]


def ref64(logits, targets, first, eps, upstream=1.0):
    """The reference's formula in fp64 -> (loss, d(upstream * loss) / dlogits), both fp64 on the CPU."""
    x = logits.detach().cpu().double().requires_grad_(True)
    mask = masks(targets.cpu(), x.shape[1], first).double()
    weit = 1 + 5 * torch.abs(F.avg_pool2d(mask, kernel_size=31, stride=1, padding=15) - mask)
    wbce = F.binary_cross_entropy_with_logits(x, mask, reduction="none")
    wbce = (weit * wbce).sum(dim=(2, 3)) / weit.sum(dim=(2, 3))
    prob = torch.sigmoid(x)
    inter = (prob * mask * weit).sum(dim=(2, 3))
    union = ((prob + mask) * weit).sum(dim=(2, 3))
    wiou = 1 - (inter + eps) / (union - inter + eps)
    loss = (wbce + wiou).mean()
    (upstream * loss).backward()
    return loss.detach(), x.grad


def window_counts(m):
    """k of csrc/structure_loss.hip: 31-tap row sums, then 31-tap column sums, of a bool mask (N, C, H, W) -> int64, zero outside."""
    N, C, H, W = m.shape
    v = m.reshape(N * C, 1, H, W).to(torch.float32)              # integers up to 961: exact in fp32
    rows = F.conv2d(v, torch.ones(1, 1, 1, WIN), padding=(0, HALO))
    k = F.conv2d(rows, torch.ones(1, 1, WIN, 1), padding=(HALO, 0))
    return k.reshape(N, C, H, W).to(torch.int64)


def restate32(logits, targets, first, eps, upstream=1.0):
    """The kernels' arithmetic in torch fp32 on the CPU -> (loss fp32, dlogits fp32)."""
    x = logits.detach().cpu().float()
    N, C = x.shape[:2]
    m = masks(targets.cpu(), C, first)
    k = window_counts(m)
    assert int(k.max()) <= WIN * WIN
    w = 5 * (torch.where(m, WIN * WIN - k, k).float() / float(WIN * WIN)) + 1
    e = torch.exp(-x.abs())
    u = 1 + e
    d = u - 1
    lp = torch.where(d == 0, e, torch.log(u) * (e / torch.where(d == 0, torch.ones_like(d), d)))
    r, er = 1 / u, e / u
    s, t = torch.where(x >= 0, r, er), torch.where(x >= 0, er, r)
    bce = x.clamp_min(0) - torch.where(m, x, torch.zeros_like(x)) + lp
    zero = torch.zeros_like(x)
    sw, sb = w.sum(dim=(2, 3)), (w * bce).sum(dim=(2, 3))
    si, sd = torch.where(m, w * s, zero).sum(dim=(2, 3)), torch.where(m, w, w * s).sum(dim=(2, 3))
    sw, sb, si, sd = (v.double() for v in (sw, sb, si, sd))      # the finalise kernel works in fp64 from the fp32 partial sums
    I, D = si + eps, sd + eps
    loss = ((sb / sw + 1 - I / D).sum() / (N * C)).float()
    c0, c1, c2 = ((v.float())[:, :, None, None] for v in (1 / sw, 1 / D, I / (D * D)))
    go = torch.tensor(upstream, dtype=torch.float32) * torch.tensor(1.0 / (N * C), dtype=torch.float32)
    a = torch.where(m, -t, s) * c0
    b = s * t * torch.where(m, c1.expand_as(s), -c2.expand_as(s))
    return loss, go * (w * (a - b))


def eager32(logits, targets, C, first, eps, upstream=1.0):
    """The eager composition in fp32 on the tensors' own device -> (loss, dlogits in the logits' dtype)."""
    from vivim_amd.structure_loss import multiclass_structure_loss, structure_loss
    x = logits.detach().requires_grad_(True)
    if first == 0:
        loss = multiclass_structure_loss(x, targets, C, eps)
    else:
        loss = structure_loss(x, (targets == first)[:, None].float(), eps)
    (upstream * loss).backward()
    return loss.detach(), x.grad


def check_loss(name, got, want64):
    e = abs(float(got) - float(want64)) / abs(float(want64))
    print(f"{name}: loss {float(got):.8f} want {float(want64):.8f} rel {e:.3e}")
    assert e <= 1e-5, f"{name}: loss {float(got)!r} against {float(want64)!r}: relative error {e:.3e} > 1e-5"
    return e


def check_norm(name, got, want64, dtype):
    want = want64.to(dtype).double()
    g = got.detach().cpu().double()
    assert torch.isfinite(g).all(), f"{name}: non-finite gradient"
    e = float((g - want).norm() / want.norm().clamp_min(1e-300))
    print(f"{name}: dlogits norm-wise {e:.3e}")
    assert e < 1e-3, f"{name}: rel-err {e:.3e} >= 1e-3"
    return e


def check_elementwise(name, got32, eager, want64):
    """|got - want| <= 2 * |eager - want| + FLOOR * max|want| per element -> (worst |got - want|, worst |eager - want|) / max|want|."""
    g, ea = got32.detach().cpu().double(), eager.detach().cpu().double()
    top = float(want64.abs().max())
    err, err_e = (g - want64).abs(), (ea - want64).abs()
    print(f"{name}: max|err| / max|want| {float(err.max()) / top:.3e} (eager {float(err_e.max()) / top:.3e})")
    bad = err > 2 * err_e + FLOOR * top
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {bad.numel()} elements outside 2 * err(eager) + floor, worst "
                                 f"{float((err - 2 * err_e).max()) / top:.3e} of max|want| against the floor {FLOOR:.1e}, first at "
                                 f"{bad.nonzero()[0].tolist()}")
    return float(err.max()) / top, float(err_e.max()) / top


def check_one_rounding(name, got16, got32, dtype):
    g16, g32 = got16.detach().cpu().double(), got32.detach().cpu().double()
    assert got16.dtype == dtype
    allow = U_ROUND[dtype] * g32.abs() * (1 + 2.0 ** -10) + 1e-5 * g32.abs() + 2.0 ** -25
    bad = (g16 - g32).abs() > allow
    assert not bool(bad.any()), (f"{name} ({dtype}): {int(bad.sum())} of {bad.numel()} elements further than one rounding from the fp32 "
                                 f"value, first at {bad.nonzero()[0].tolist()}")
