"""CPU references for the v3 block and its direction maps, shared by tests/test_v3_block_reference.py, test_gpu_dirmap.py and
test_gpu_v3_block.py.  Everything here is plain torch in float64 on the CPU; nothing imports the product.

    map_stack / map_unstack     the three direction maps of csrc/dirmap.hip as index operations: identity, flip(-1) and the
                                frame interleave t*hw+p <-> p*nf+t by reshape / transpose
    v3_forward64                the v3 block of oracle/ref_torch.py:mamba_v3_forward_ref, float64 throughout (ref_torch casts to
                                fp32 inside the scan), the recurrence walked over unbind(-1) pieces: indexing [..., t] inside
                                the loop makes autograd's backward of an L = 2600 block take minutes instead of seconds
    v3_reference                forward + autograd gradients of a loss, as the dict block_errors compares
    block_errors                y, dx: the worst per-token relative error max_t ||got_t - ref_t|| / ||ref_t|| (a Frobenius norm over
                                the whole tensor hides a misplaced tile, the worst token does not); every parameter gradient: the
                                norm-wise relative error of that tensor (the three directions' parameters are separate tensors)"""
import torch
import torch.nn.functional as F


# ---- direction maps

def interleave(x, nf):
    """(..., L) frame-major t*hw+p -> pixel-major p*nf+t."""
    L = x.shape[-1]
    return x.reshape(*x.shape[:-1], nf, L // nf).transpose(-1, -2).reshape(*x.shape[:-1], L)


def deinterleave(x, nf):
    """The inverse of `interleave`: pixel-major p*nf+t -> frame-major t*hw+p."""
    L = x.shape[-1]
    return x.reshape(*x.shape[:-1], L // nf, nf).transpose(-1, -2).reshape(*x.shape[:-1], L)


def map_stack(x, nf):
    """(..., L) -> the three directions (identity, time reversal, frame interleave) of the rounded input, in float64."""
    x = x.detach().double().cpu()
    return x, x.flip(-1), interleave(x, nf)


def map_unstack(a, b, c, nf):
    """The three directions' tensors brought back to frame-major token order, in float64: what the gather sums."""
    a, b, c = (t.detach().double().cpu() for t in (a, b, c))
    return a, b.flip(-1), deinterleave(c, nf)


# ---- the v3 block

def _scan64(u, delta, A, Bm, Cm, D, z, delta_bias):
    """Sequential selective scan with input-dependent B and C, softplus(delta + bias), D and the silu(z) gate.
    u, delta, z (b, d, l); A (d, n); Bm, Cm (b, n, l); D, delta_bias (d,) -- all float64."""
    dt = F.softplus(delta + delta_bias[:, None])
    decay = torch.exp(dt[:, :, None, :] * A[None, :, :, None])                    # (b, d, n, l)
    drive = Bm[:, None] * (dt * u)[:, :, None, :]
    h = u.new_zeros(u.shape[0], u.shape[1], A.shape[1])
    ys = []
    for a_t, x_t, c_t in zip(decay.unbind(-1), drive.unbind(-1), Cm.unbind(-1)):
        h = a_t * h + x_t
        ys.append((h * c_t[:, None]).sum(-1))
    y = torch.stack(ys, dim=-1) + u * D[:, None]
    return y * F.silu(z)


def _inner64(xz, p, sfx, n):
    """conv1d + SiLU -> x_proj -> dt_proj -> scan of one direction; xz (b, 2 d_inner, l) -> (b, d_inner, l)."""
    b, _, l = xz.shape
    x, z = xz.chunk(2, dim=1)
    w = p[f"conv1d{sfx}.weight"]                                                  # (d, 1, width)
    d, width = w.shape[0], w.shape[-1]
    x = F.silu(F.conv1d(x, w, p.get(f"conv1d{sfx}.bias"), padding=width - 1, groups=d)[..., :l])
    dtw = p[f"dt_proj{sfx}.weight"]
    r = dtw.shape[1]
    x_dbl = F.linear(x.transpose(1, 2).reshape(b * l, d), p[f"x_proj{sfx}.weight"])          # (b l, r + 2n)
    delta = (dtw @ x_dbl[:, :r].t()).reshape(d, b, l).transpose(0, 1)
    Bm = x_dbl[:, r:r + n].reshape(b, l, n).transpose(1, 2)
    Cm = x_dbl[:, r + n:].reshape(b, l, n).transpose(1, 2)
    return _scan64(x, delta, -torch.exp(p[f"A{sfx}_log"]), Bm, Cm, p[f"D{sfx}"], z, p[f"dt_proj{sfx}.bias"])


def v3_forward64(hidden, p, nframes):
    """The v3 block on float64 `hidden` (b, l, d_model) and a dict `p` of float64 parameters under the module's state-dict
    names: in_proj, three directions of conv + SiLU / x_proj / dt_proj / scan with D and the z gate, their mean, out_proj."""
    assert hidden.dtype == torch.float64 and all(v.dtype == torch.float64 for v in p.values())
    b, l, _ = hidden.shape
    xz = p["in_proj.weight"] @ hidden.reshape(b * l, -1).t()
    if "in_proj.bias" in p:
        xz = xz + p["in_proj.bias"][:, None]
    xz = xz.reshape(-1, b, l).transpose(0, 1)                                     # (b, 2 d_inner, l)
    n = p["A_log"].shape[1]
    out = _inner64(xz, p, "", n)
    out_b = _inner64(xz.flip(-1), p, "_b", n).flip(-1)
    out_s = deinterleave(_inner64(interleave(xz, nframes), p, "_s", n), nframes)
    y = (out + out_b + out_s).transpose(1, 2) / 3
    return F.linear(y, p["out_proj.weight"], p.get("out_proj.bias"))


def v3_reference(hidden, params, nframes, dout=None):
    """Forward and autograd backward of the float64 block on float64 copies of `hidden` and `params` (name -> tensor).
    The loss is y.square().mean(), or <y, dout> when `dout` is given.  -> {"y", "dx", "grads": {name: tensor}}, float64."""
    x = hidden.detach().double().cpu().clone().requires_grad_(True)
    p = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in params.items()}
    y = v3_forward64(x, p, nframes)
    if dout is None:
        y.square().mean().backward()
    else:
        y.backward(dout.detach().double().cpu())
    return {"y": y.detach(), "dx": x.grad, "grads": {k: v.grad for k, v in p.items()}}


def token_error(got, ref):
    """max over the tokens of ||got_t - ref_t|| / ||ref_t|| for (B, L, d_model) tensors."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    return float(((g - r).norm(dim=-1) / r.norm(dim=-1).clamp_min(1e-300)).max())


def block_errors(got, ref):
    """`got`, `ref`: {"y", "dx", "grads": {name: tensor}} -> {"y": ..., "dx": ..., "grad:<name>": ...}: per-token worst
    relative error of y and dx, norm-wise relative error of every parameter gradient of `ref`."""
    out = {"y": token_error(got["y"], ref["y"]), "dx": token_error(got["dx"], ref["dx"])}
    for k, r in ref["grads"].items():
        g = got["grads"][k].detach().double().cpu()
        out["grad:" + k] = float((g - r).norm() / r.norm().clamp_min(1e-300))
    return out
