"""What tests/test_gpu_add_norm_tm.py (the kernels) and tests/test_abi_add_norm_tm.py (a torch fp32 restatement of the kernels'
arithmetic, on the CPU) share: the inputs, the fp64 reference and the bounds of the token-major residual add + LayerNorm / RMSNorm.

The reference is fp64 on the CPU from the same rounded inputs, and takes THE SUM THE OP RETURNED (res_new) for the norm and its
gradients: the kernels norm the row as stored.

Bounds:
    res_new  per element  |got - want| <= 2 * 2^-24 * (|res| + |scale * branch|) + u(res dtype) * |want|
             (two fp32 roundings at most -- the product, the sum -- then the one rounding to the stored type)
    y        per row      fp32 < 2e-6 (+ 4 * 2^-24 * |mean| / std for LayerNorm on the hard family), 16-bit < 4e-3
    dres_in, dbranch  per row, by their own dtype   fp32 < 1e-5, 16-bit < 4e-3; rows with scale == 0 have dbranch exactly 0
    dweight, dbias    over the vector   < 1e-4"""
import torch

from fp64_bounds import U_ROUND

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
PAIRS = [(F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32)]          # (branch = y dtype, residual dtype)
FAMILIES = {"base": (1.7, 0.4), "hard": (1.0, 30.0)}
# (layout, shape): plain rows; a 3-D tensor whose samples (5 rows) straddle a wave's 8 rows; a channel slice of wider rows for the
# branch / for the residual; a view one element into its storage for the branch / for the residual (the element path)
SHAPES = [("rows", (5, 8)), ("rows", (37, 64)), ("rows", (9, 36)), ("rows", (67, 320)), ("rows", (19, 512)), ("rows", (3, 1000)),
          ("rows", (1, 64)), ("rows", (7, 63)), ("rows", (3, 5, 64)), ("branch_slice", (3, 5, 64)), ("res_slice", (3, 5, 64)),
          ("branch_offset", (7, 64)), ("res_offset", (7, 64))]
BIG = ("rows", (4133, 512))                              # fp32 only: more than 1024 workgroups -- the slot cap, the grid-stride loop
# (rms, bias, eps, scale): every flag both ways, every scale kind with both norms
COMBOS = [(False, True, 1e-5, None), (False, False, 1e-6, "ones"), (False, True, 1e-6, "drop"),
          (True, True, 1e-5, "drop"), (True, False, 1e-6, None), (True, False, 1e-5, "ones")]


def name(dt):
    return str(dt).replace("torch.", "")


def _tensor(gen, shape, dtype, mul, add, how):
    C = shape[-1]
    if how == "slice":
        return torch.randn(*shape[:-1], C + 8, generator=gen).mul_(mul).add_(add).to(dtype)[..., :C]
    if how == "offset":
        n = 1
        for d in shape:
            n *= d
        return torch.randn(n + 1, generator=gen).mul_(mul).add_(add).to(dtype)[1:].view(shape)
    return torch.randn(*shape, generator=gen).mul_(mul).add_(add).to(dtype)


def scale_of(kind, samples):
    if kind is None:
        return None
    if kind == "ones":
        return torch.ones(samples)
    return torch.tensor([1.25, 0.0] * samples)[:samples]             # 1 / 0.8 for a kept sample, 0 for a dropped one, in turn


def inputs(layout, shape, family, btype, rtype, seed):
    """CPU tensors, already rounded to the I/O types: res, branch (views where the layout says so), weight, bias, dy, dres."""
    gen = torch.Generator().manual_seed(seed)
    mul, add = FAMILIES[family]
    C = shape[-1]
    how = {"branch_slice": ("rows", "slice"), "res_slice": ("slice", "rows"), "branch_offset": ("rows", "offset"),
           "res_offset": ("offset", "rows")}.get(layout, ("rows", "rows"))
    res = _tensor(gen, shape, rtype, mul, add, how[0])
    branch = _tensor(gen, shape, btype, 1.3, 0.2, how[1])
    w = torch.randn(C, generator=gen) * 0.5 + 1.0
    b = torch.randn(C, generator=gen) * 0.3
    dy = torch.randn(*shape, generator=gen).to(btype)
    dres = torch.randn(*shape, generator=gen).to(rtype)
    return {"res": res, "branch": branch, "w": w, "b": b, "dy": dy, "dres": dres}


def _expand(scale, like):
    """scale (samples,) -> one factor per row, broadcastable against `like` (samples, ..., C)."""
    if scale is None:
        return torch.ones((), dtype=torch.float64)
    return scale.double().view((-1,) + (1,) * (like.dim() - 1))


def norm64(h, w, b, eps, rms):
    if rms:
        y = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps) * w
    else:
        mean = h.mean(-1, keepdim=True)
        y = (h - mean) * torch.rsqrt((h - mean).pow(2).mean(-1, keepdim=True) + eps) * w
    return y if b is None else y + b


def reference(res_new, res, branch, scale, w, b, dy, dres, eps, rms):
    """fp64: the exact sum, and the norm of `res_new` (the sum as the op stored it) with the gradients dy and dres send back."""
    s = _expand(scale, branch)
    want_sum = s * branch.double() if res is None else res.double() + s * branch.double()
    mag = (s * branch.double()).abs() + (0 if res is None else res.double().abs())
    out = {"sum": want_sum, "sum_mag": mag, "h": res_new.double()}
    if w is None:
        out["dres_in"] = dres.double()
        out["dbranch"] = s * dres.double()
        return out
    h = res_new.double().clone().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    b64 = None if b is None else b.double().requires_grad_(True)
    y = norm64(h, w64, b64, eps, rms)
    out["y"] = y.detach()
    dh = torch.zeros_like(h)
    if dy is not None:
        y.backward(dy.double())
        dh, out["dw"], out["db"] = h.grad, w64.grad, None if b is None else b64.grad
    if dres is not None:
        dh = dh + dres.double()
    out["dres_in"], out["dbranch"] = dh, s * dh
    return out


def emulate(res, branch, scale, w, b, dy, dres, eps, rms):
    """The kernels' arithmetic restated with torch fp32 ops on the CPU: the sum rounded once to the residual dtype, the norm of the
    stored row (the mean first, then the squared differences; RMS skips the mean), today's backward formula plus dres."""
    s = torch.ones(()) if scale is None else scale.view((-1,) + (1,) * (branch.dim() - 1))
    res_new = (res.float() + s * branch.float()).to(res.dtype)
    got = {"res_new": res_new}
    if w is None:
        got["dbranch"] = (s * dres.float()).to(branch.dtype)
        return got
    h = res_new.float()
    mean = torch.zeros_like(h[..., :1]) if rms else h.mean(-1, keepdim=True)
    d = h - mean
    rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    y = d * rstd * w
    got["y"] = (y if b is None else y + b).to(branch.dtype)
    xh, g = d * rstd, dy.float() * w
    s1 = torch.zeros_like(mean) if rms else g.mean(-1, keepdim=True)
    dh = rstd * (g - s1 - xh * (g * xh).mean(-1, keepdim=True)) + dres.float()
    got["dres_in"], got["dbranch"] = dh.to(res.dtype), (s * dh).to(branch.dtype)
    C = h.shape[-1]
    got["dw"], got["db"] = (dy.float() * xh).reshape(-1, C).sum(0), (None if b is None else dy.float().reshape(-1, C).sum(0))
    return got


def _rows_ratio(got, want, bound):
    """max over the rows of (||got - want|| / ||want||) / bound; a row whose reference is all zero has to be zero."""
    C = want.shape[-1]
    g, r = got.detach().double().cpu().reshape(-1, C), want.reshape(-1, C)
    err, nrm = (g - r).norm(dim=1), r.norm(dim=1)
    zero = nrm == 0
    assert bool((err[zero] == 0).all()), "a row whose reference is all zero is not zero"
    rel = torch.where(zero, torch.zeros_like(err), err / nrm.clamp_min(1e-300))
    return float((rel / bound).max())


def sum_ratio(res_new, ref, rtype):
    """max over the elements of |res_new - want| / bound."""
    bound = 2 * 2.0 ** -24 * ref["sum_mag"] + U_ROUND[rtype] * ref["sum"].abs()
    err = (res_new.detach().double().cpu() - ref["sum"]).abs()
    assert bool((err[bound == 0] == 0).all())
    return float((err / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0


def ratios(got, ref, scale, btype, rtype, family, eps, rms):
    """err / bound of every bound in this module's docstring for one call -> dict; `got` holds what the op (or `emulate`) gave."""
    out = {"res_new": sum_ratio(got["res_new"], ref, rtype)}
    grad_tol = {True: 1e-5, False: 4e-3}
    if "y" in got:
        C = ref["h"].shape[-1]
        y_tol = torch.full((ref["h"].numel() // C,), 2e-6 if btype == F32 else 4e-3, dtype=torch.float64)
        if btype == F32 and family == "hard" and not rms:
            rows = ref["h"].reshape(-1, C)
            y_tol += 4 * 2.0 ** -24 * rows.mean(dim=1).abs() / rows.var(dim=1, unbiased=False).add(eps).sqrt()
        out["y"] = _rows_ratio(got["y"], ref["y"], y_tol)
    if got.get("dres_in") is not None:
        out["dres_in"] = _rows_ratio(got["dres_in"], ref["dres_in"], grad_tol[rtype == F32])
    if got.get("dbranch") is not None:
        out["dbranch"] = _rows_ratio(got["dbranch"], ref["dbranch"], grad_tol[btype == F32])
        if scale is not None:                            # a dropped sample's rows: exactly 0
            dropped = got["dbranch"].detach().cpu()[scale.cpu() == 0]
            assert bool((dropped == 0).all()), "dbranch of a dropped sample is not exactly 0"
    for k in ("dw", "db"):
        if got.get(k) is not None:
            want = ref[k]
            out[k] = float((got[k].detach().double().cpu() - want).norm() / want.norm().clamp_min(1e-30)) / 1e-4
    return out
