"""What tests/test_gpu_fused_optimizer.py (the kernels) and tests/test_abi_fused_optimizer.py (a torch fp32 restatement of the
kernels' arithmetic, on the CPU) share: the tensor lists, the input families, the fp64 reference and the bounds of the fused
clip + AdamW step (csrc/optimizer.hip).

The reference is the definition in fp64 on the CPU, from the fp32 state the op started from:
    g' = g * factor;  m' = m + (1 - b1)(g' - m);  v' = b2 v + (1 - b2) g'^2
    p' = p (1 - lr wd) - (lr / bc1) m' / (sqrt(v') / bc2s + eps),  bc1 = 1 - b1^t,  bc2s = sqrt(1 - b2^t)
`factor` is the fp32 value the update read from the record -- part of the state it started from -- and is itself pinned to 4u
of its fp64 value, inv_scale * min(1, max_norm / (norm + 1e-6)).

Bounds per element, u = 2^-24, from the operation count of the kernel:
    m:  g * factor (u |g'|), g' - m (u |g' - m|), (1 - b1) rounded once (u |g' - m|), one fma (u |m'|), and |g' - m| and |m'|
        are at most |m| + |g'|:  4u (|m| + |g'|)  for any b1 (1.1 u (|m| + |g'|) at b1 = 0.9)
    v:  (1 - b2) and b2 rounded once, g * factor twice, two products, one fma: 7 roundings of terms that are all >= 0 and add up
        to v' -- first order 7u v', with the second-order terms  8u v' + 1e-37  (the absolute term: v' that underflows)
    p:  p * decay and the fma: 2u |p| + u |p'|;  lr / bc1 (bc1 rounded, the division: 2u), m' / denom (u), denom = sqrt (u),
        / bc2s (bc2s rounded, the division: 2u), + eps (u, eps rounded: u), and m' and v' as above (v' under the root: halved):
        about 12 u (lr / bc1) |m'| / denom, and |m'| <= |m| + |g'|:  u (4 |p| + 16 (lr / bc1) (|m| + |g'|) / denom)
Norm: a thread adds 16 squares in a chain, then 6 wave steps, 3 workgroup adds, and the slots in fp64; the square itself is
two roundings.  0.5 * (chain + 16) u relative on the norm covers any chain up to 256: 0.5 * (256 + 16) u = 8.1e-6."""
import math

import torch

U = 2.0 ** -24
CHUNK, MAX_TENSORS, THREADS, VEC = 4096, 248, 256, 4           # VIVIM_OPT_CHUNK, VIVIM_OPT_MAX_TENSORS; the workgroup, a 16-byte access
LR, BETAS, EPS, WD = 1e-3, (0.9, 0.999), 1e-8, 1e-2
NORM_BOUND = 0.5 * (256 + 16) * U
STEPS = 12
G_SCALES = (1e-3, 1.0, 65.5)
P_FAMILIES = {"base": 0.0, "offset": 30.0}                      # p = 0.05 randn (+ 30)
FACTORS = ("one", "scaled", "clip")                             # factor 1 | 2^-16 through the loss scale | a clip below 1
CLIP_AT = 0.37                                                  # max_norm as a fraction of the true norm

# list A: (shape, layout).  "p1" / "g1" / "m1" / "v1": that tensor is a view one element into its storage; "row": row 1 of a
# stacked (3, 5, 7) buffer (140 bytes in: not 16-byte aligned)
LIST_A = [((), None), ((1,), None), ((3,), None), ((7,), None), ((64,), None), ((255,), None), ((257,), None),
          ((CHUNK - 1,), None), ((CHUNK,), None), ((CHUNK + 1,), None), ((2 * CHUNK + 5,), None),
          ((CHUNK + 5,), "p1"), ((CHUNK + 5,), "g1"), ((CHUNK + 5,), "m1"), ((CHUNK + 5,), "v1"), ((5, 7), "row")]


def list_b_shapes():
    """1000 tensors of 1 .. 33 elements: five kernel-argument tables."""
    gen = torch.Generator().manual_seed(77)
    return [((int(n),), None) for n in torch.randint(1, 34, (1000,), generator=gen)]


def shapes_of(which):
    return LIST_A if which == "A" else list_b_shapes()


def numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def params_cpu(which, family, seed):
    """-> list of fp32 CPU tensors, the parameters' start values."""
    gen = torch.Generator().manual_seed(seed)
    return [0.05 * torch.randn(shape, generator=gen) + P_FAMILIES[family] for shape, _ in shapes_of(which)]


def grads_cpu(which, step, seed):
    """-> list of fp32 CPU tensors: randn x {1e-3, 1, 65.5} by step, every 7th element zero on every third step."""
    gen = torch.Generator().manual_seed(1000 * seed + step)
    out = []
    for shape, _ in shapes_of(which):
        g = torch.randn(shape, generator=gen) * G_SCALES[step % 3]
        if step % 3 == 2:
            g.view(-1)[::7] = 0.0
        out.append(g)
    return out


def flat64(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors]).double().cpu()


def norm64(grads, inv_scale=1.0):
    return float((flat64(grads) * inv_scale).square().sum().sqrt())


def factor64(norm, inv_scale, max_norm):
    """-> (clip, factor) of the definition, in fp64."""
    clip = 1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))
    return clip, inv_scale * clip


def reference(p, g, m, v, factor, t, lr=LR, betas=BETAS, eps=EPS, wd=WD):
    """fp64 flat tensors and the step count AFTER this step -> (p', m', v'), (bound p, bound m, bound v)."""
    b1, b2 = betas
    gp = g * factor
    m2 = m + (1.0 - b1) * (gp - m)
    v2 = b2 * v + (1.0 - b2) * gp * gp
    ss = lr / (1.0 - b1 ** t)
    denom = v2.sqrt() / math.sqrt(1.0 - b2 ** t) + eps
    p2 = p * (1.0 - lr * wd) - ss * m2 / denom
    reach = m.abs() + gp.abs()
    return (p2, m2, v2), (U * (4.0 * p.abs() + 16.0 * ss * reach / denom), 4.0 * U * reach, 8.0 * U * v2 + 1e-37)


def factor_sensitivity(g, m, v, factor, t, lr=LR, betas=BETAS, eps=EPS):
    """|dp'/dfactor| * factor, |dm'/dfactor| * factor, |dv'/dfactor| * factor per element, fp64: what a RELATIVE error of the
    factor does to the results, to first order (the second order is below 1e-10 relative for the errors it is used with)."""
    b1, b2 = betas
    gp = g * factor
    m2 = m + (1.0 - b1) * (gp - m)
    v2 = b2 * v + (1.0 - b2) * gp * gp
    bc2s = math.sqrt(1.0 - b2 ** t)
    ss = lr / (1.0 - b1 ** t)
    denom = v2.sqrt() / bc2s + eps
    dm = (1.0 - b1) * gp.abs()
    dv = 2.0 * (1.0 - b2) * gp * gp
    ddenom = torch.where(v2 > 0, dv / (2.0 * v2.sqrt().clamp_min(1e-300) * bc2s), torch.zeros_like(v2))
    return ss * (dm / denom + m2.abs() * ddenom / denom ** 2), dm, dv


def worst(got, want, bound):
    """max over the elements of |got - want| / bound (fp64 flat tensors)."""
    return float(((got - want).abs() / bound).max()) if got.numel() else 0.0


# ---- the kernels' arithmetic in torch fp32 on the CPU
def _f32(x):
    return torch.tensor(x, dtype=torch.float64).float()


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in fp64; the sum is rounded to 53 bits and then to 24 (a double rounding
    differs from the fused one only in rare ties)."""
    return (a.double() * b.double() + c.double()).float()


def restate_update(p, g, m, v, factor, bc1, bc2s, lr=LR, betas=BETAS, eps=EPS, wd=WD):
    """opt_adamw_kernel on fp32 CPU tensors; factor, bc1, bc2s are fp32 scalars (tensors) as the record holds them."""
    b1, b2 = betas
    omb1, b2f, omb2, epsf, decay, lrf = _f32(1.0 - b1), _f32(b2), _f32(1.0 - b2), _f32(eps), _f32(1.0 - lr * wd), _f32(lr)
    gs = g * factor
    mn = _fma(omb1, gs - m, m)
    vn = _fma(b2f, v, (omb2 * gs) * gs)
    denom = vn.sqrt() / bc2s + epsf
    pn = _fma(-(lrf / bc1), mn / denom, p * decay)
    return pn, mn, vn


def restate_sumsq(grads, inv_scale, iters=CHUNK // (THREADS * VEC)):
    """opt_grad_stats_kernel + the slot sum: per tensor and chunk of 256 * 4 * iters elements, thread j adds the squares of
    elements (it * 256 + j) * 4 + k in (it, k) order in one fp32 chain of 4 * iters fmas, a butterfly over each 64-lane wave, the
    four waves in order; the slots are added in fp64.  iters = 64 is a chain of 256."""
    chunk = THREADS * VEC * iters
    inv = _f32(inv_scale)
    total = torch.zeros((), dtype=torch.float64)
    for g in grads:
        flat = g.detach().reshape(-1).float()
        blocks = -(-flat.numel() // chunk)
        x = torch.zeros(blocks * chunk)
        x[:flat.numel()] = flat
        x = (x * inv).view(blocks, iters, THREADS, VEC)
        acc = torch.zeros(blocks, THREADS)
        for it in range(iters):
            for k in range(VEC):
                acc = _fma(x[:, it, :, k], x[:, it, :, k], acc)
        acc = acc.view(blocks, THREADS // 64, 64)
        lanes = torch.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, :, lanes ^ off]
        s = acc[:, 0, 0]
        for w in range(1, THREADS // 64):
            s = s + acc[:, w, 0]
        total = total + s.double().sum()
    return total


def bias_corrections(t, betas=BETAS):
    """(bc1, bc2s) as the record holds them after step t: fp64, rounded once."""
    return _f32(1.0 - betas[0] ** t), _f32(math.sqrt(1.0 - betas[1] ** t))
