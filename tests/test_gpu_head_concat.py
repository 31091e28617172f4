"""GPU: vivim_amd.head_concat.upsample_concat (csrc/head_concat.hip) against the definition, per map slice and elementwise, forward
and backward, in fp32 / fp16 / bf16 with masks on none, some and all maps; dropped elements; element accesses at odd offsets; bytes
outside the written slices; the transpose identity; bit-repeatability; the drawn masks; no write outside the buffers (VIVIM_GUARD
child); and the head inside Vivim against an fp64 copy that replays the masks.

The reference and the bounds are head_concat_cases.py's (its docstring derives them); they are derived, not measured.  The measured
maxima, as shares of the bounds, go to the parity log that conftest.py keeps.

The head inside Vivim (train mode, fp32 and bf16 autocast; feature_dropout and the decoder's dropout at p = 0; draw_keep and the
stock route's F.dropout(p = dropout_rate / 2) replaced by the same recorded masks): the logits and every head parameter's gradient of
the stock and the new route against the fp64 copy, err(new) <= 2 err(stock) + FLOOR max|want| per tensor -- the rule of
tests/test_gpu_structure_loss.py.  FLOOR = 1.5e-5 is 4 x the worst error of the fp32 head on the CPU on these inputs, 3.67e-6 of
max|want| (head_concat_cases.FLOOR; tests/test_abi_head_concat.py recomputes it)."""
import copy
import math
import os
import subprocess
import sys

import pytest
import torch

import head_concat_cases as hc
from conftest import _PARITY_LOG, ROOT
from test_gpu_upsample import U

pytestmark = pytest.mark.gpu


def _log(test, what, dtype, share):
    try:
        os.makedirs(os.path.dirname(_PARITY_LOG), exist_ok=True)
        with open(_PARITY_LOG, "a") as f:
            f.write(f"{test}\t{what}\t{str(dtype).replace('torch.', '')}\tmax_err_over_bound={share:.3e}\n")
    except OSError:
        pass
    print(f"{test} {what} {dtype}: max err / bound {share:.3e}")


def _cl(t, cuda):
    return t.to(cuda).contiguous(memory_format=torch.channels_last)


def _inputs(c, cuda):
    return [_cl(m, cuda) for m in c["maps"]], _cl(c["go"], cuda), [None if k is None else k.to(cuda) for k in c["keep"]]


def _run(maps, go, size, p, keep):
    from vivim_amd.head_concat import upsample_concat
    maps = [m.detach().requires_grad_(True) for m in maps]
    y = upsample_concat(maps, size, p, keep)
    y.backward(go)
    return y.detach(), [m.grad for m in maps]


def _calls(fn):
    """fn() and the names of the C-ABI calls it made (the _lib profile hook)."""
    from vivim_amd import _lib
    _lib.profile_begin(all_kernels=True)
    try:
        out = fn()
    finally:
        names = [r[0] for r in _lib.profile_end()]
    return out, names


@pytest.mark.parametrize("name,dt,masks", hc.GRID)
def test_values_and_gradients(name, dt, masks, cuda):
    from vivim_amd import head_concat
    c = hc.case(name, dt, masks)
    maps, go, keep = _inputs(c, cuda)
    assert head_concat.supported(maps, c["size"], keep)
    (y, dxs), names = _calls(lambda: _run(maps, go, c["size"], c["p"], keep))
    assert names == ["vivim_head_concat_fwd", "vivim_head_concat_bwd"]                 # one launch each way, whatever the map count
    N, total, (OH, OW) = maps[0].shape[0], go.shape[1], c["size"]
    assert y.dtype == c["dtype"] and y.shape == (N, total, OH, OW) and y.permute(0, 2, 3, 1).is_contiguous()
    assert all(dx.dtype == c["dtype"] and dx.shape == m.shape and dx.permute(0, 2, 3, 1).is_contiguous() for dx, m in zip(dxs, maps))
    assert torch.isfinite(y.float()).all() and all(torch.isfinite(dx.float()).all() for dx in dxs)
    wf, wb = hc.check(c, y, dxs, f"head_concat[{name} {dt} {masks}]")
    _log(f"head_concat[{name}-{masks}]", "y", c["dtype"], wf)
    _log(f"head_concat[{name}-{masks}]", "dx", c["dtype"], wb)
    for s, k in enumerate(keep):
        if k is not None:                                                              # a dropped element is exactly 0
            r, C = c["refs"][s], maps[s].shape[1]
            assert bool((y[:, r["off"]:r["off"] + C][k.permute(0, 3, 1, 2) == 0] == 0).all())


def _odd_view(t):
    """The same values as a channels-last view one element into a larger buffer: misaligned for every 16-byte access."""
    N, C, H, W = t.shape
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(N, H, W, C).permute(0, 3, 1, 2)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.stride() == t.stride()
    return v


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("which", ["map", "grad"])
def test_odd_element_offset_takes_element_accesses(which, dt, cuda):
    """ratios: every map fills 16-byte vectors when aligned.  One map, or the output gradient, one element into its storage moves
    that map's (the backward's) accesses to elements: the same bits (the kernels spell their fused multiply-adds out), inside the
    bounds."""
    c = hc.case("ratios", dt, "some")
    maps, go, keep = _inputs(c, cuda)
    y0, dx0 = _run(maps, go, c["size"], c["p"], keep)
    if which == "map":
        maps[2] = _odd_view(maps[2])
    else:
        go = _odd_view(go)
    y1, dx1 = _run(maps, go, c["size"], c["p"], keep)
    assert torch.equal(y0, y1) and all(torch.equal(a, b) for a, b in zip(dx0, dx1))
    hc.check(c, y1, dx1, f"head_concat at an odd offset ({which})")


def test_a_gradient_that_is_not_dense_channels_last_is_made_so(cuda):
    c = hc.case("odd_c", "fp32", "all")
    maps, go, keep = _inputs(c, cuda)
    y0, dx0 = _run(maps, go, c["size"], c["p"], keep)
    planes = go.contiguous()                                                           # NCHW
    wide = torch.zeros(go.shape[0], go.shape[1] + 3, *go.shape[2:], device=cuda).to(go.dtype).contiguous(memory_format=torch.channels_last)
    wide[:, :go.shape[1]] = go
    for g in (planes, wide[:, :go.shape[1]]):
        assert g.stride() != go.stride()
        y1, dx1 = _run(maps, g, c["size"], c["p"], keep)
        assert torch.equal(y0, y1) and all(torch.equal(a, b) for a, b in zip(dx0, dx1))


@pytest.mark.parametrize("name,dt", [("ratios", "bf16"), ("odd_c", "fp32")])
def test_a_dropped_element_contributes_exactly_nothing(name, dt, cuda):
    """The gradient is NaN at every dropped position of the masked maps: dx has the bits of the finite run."""
    c = hc.case(name, dt, "zero")
    maps, go, keep = _inputs(c, cuda)
    _, dx0 = _run(maps, go, c["size"], c["p"], keep)
    bad = go.clone()
    for s, k in enumerate(keep):
        r, C = c["refs"][s], maps[s].shape[1]
        bad[:, r["off"]:r["off"] + C][k.permute(0, 3, 1, 2) == 0] = float("nan")
    assert int(torch.isnan(bad).sum()) >= bad[:, :maps[0].shape[1]].numel()           # map 0's mask is all zero
    _, dx1 = _run(maps, bad, c["size"], c["p"], keep)
    assert all(torch.equal(a, b) for a, b in zip(dx0, dx1)) and bool((dx1[0] == 0).all())


@pytest.mark.parametrize("dt,gap", [("bf16", 8), ("fp32", 3)])
def test_bytes_outside_the_written_slices_keep_their_fill(dt, gap, cuda):
    """Op level: the forward into an out_pixel_stride wider than sum C_s, the blocks apart from each other -- the gaps keep their
    fill, the blocks have the op's bits.  gap = 8 keeps bf16 on the vector path, gap = 3 takes fp32 off it."""
    import ctypes
    from vivim_amd import _lib
    c = hc.case("ratios", dt, "some")
    maps, go, keep = _inputs(c, cuda)
    y0, _ = _run(maps, go, c["size"], c["p"], keep)
    N, (OH, OW) = maps[0].shape[0], c["size"]
    stride = go.shape[1] + gap * (len(maps) + 1)
    out = torch.full((N, OH, OW, stride), 77.0, device=cuda).to(c["dtype"])
    P = _lib.HeadConcatParams()
    P.struct_bytes, P.batch, P.n_maps, P.itype = ctypes.sizeof(P), N, len(maps), _lib.ITYPE[c["dtype"]]
    P.out_h, P.out_w, P.out, P.out_batch_stride, P.out_pixel_stride = OH, OW, out.data_ptr(), out.stride(0), stride
    covered = torch.zeros(stride, dtype=torch.bool)
    for s, m in enumerate(maps):
        off = c["refs"][s]["off"] + gap * (s + 1)
        P.map_c[s], P.map_h[s], P.map_w[s], P.chan_off[s], P.scale[s] = m.shape[1], m.shape[2], m.shape[3], off, c["refs"][s]["scale"]
        P.maps[s], P.map_batch_stride[s] = m.data_ptr(), m.stride(0)
        if keep[s] is not None:
            P.keep[s], P.keep_batch_stride[s] = keep[s].data_ptr(), keep[s].stride(0)
        covered[off:off + m.shape[1]] = True
    _lib.launch("vivim_head_concat_fwd", P, cuda)
    torch.cuda.synchronize()
    assert int((~covered).sum()) == gap * (len(maps) + 1)
    assert bool((out[..., ~covered.to(cuda)] == 77.0).all())
    assert torch.equal(out[..., covered.to(cuda)].permute(0, 3, 1, 2), y0)


@pytest.mark.parametrize("name,masks", [("ratios", "some"), ("odd_c", "all"), ("wide", "none")])
def test_transpose_identity_fp32(name, masks, cuda):
    """<y, g> and sum_s <x_s, dx_s> agree to sum_s (T_s + 10) u sum|x_s| S_s: forward and backward share one tap function, one mask
    and one scale (test_gpu_upsample's (T + 8) u with the two more roundings of the products by the scale)."""
    c = hc.case(name, "fp32", masks)
    maps, go, keep = _inputs(c, cuda)
    y, dxs = _run(maps, go, c["size"], c["p"], keep)
    a = float((y.double().cpu() * c["go"].double()).sum())
    b = sum(float((dx.double().cpu() * m.double()).sum()) for dx, m in zip(dxs, c["maps"]))
    tol = sum((r["T"] + 10) * U * float((m.double().abs() * r["S"]).sum()) for r, m in zip(c["refs"], c["maps"]))
    print(f"transpose[{name}-{masks}]: <y, g> = {a:.9e}, sum <x, dx> = {b:.9e}, |difference| {abs(a - b):.3e}, tolerance {tol:.3e}")
    assert abs(a - b) <= tol


@pytest.mark.parametrize("name,dt", [("ratios", "bf16"), ("odd_c", "fp32"), ("c768", "bf16")])
def test_equal_bits_with_and_without_the_strict_flag(name, dt, cuda):
    c = hc.case(name, dt, "some")
    maps, go, keep = _inputs(c, cuda)
    run = lambda: _calls(lambda: _run(maps, go, c["size"], c["p"], keep))      # noqa: E731
    (y0, dx0), names0 = run()
    junk = torch.full((16 << 20,), float("nan"), device=cuda)                  # the next buffers come back from the allocator full of NaN
    del junk
    (y1, dx1), _ = run()
    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        (y2, dx2), names2 = run()
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=prev_warn)
    assert names0 == names2 == ["vivim_head_concat_fwd", "vivim_head_concat_bwd"]      # the same kernels under the flag
    for y, dx in ((y1, dx1), (y2, dx2)):
        assert torch.equal(y0, y) and all(torch.equal(a, b) for a, b in zip(dx0, dx))


def test_drawn_masks_are_bernoulli(cuda):
    """With p given and no masks the op draws them through head_concat.draw_keep: uint8 of 0 / 1, one per map with a probability, and
    the kept share of each is within 6 standard deviations of 1 - p for its element count."""
    from vivim_amd import head_concat
    c = hc.case("c768", "bf16", "some")
    maps, go, _ = _inputs(c, cuda)
    drawn, orig = [], head_concat.draw_keep

    def recording(shape, p, device):
        drawn.append((p, orig(shape, p, device)))
        return drawn[-1][1]

    head_concat.draw_keep = recording
    try:
        torch.manual_seed(0)
        y, _ = _run(maps, go, c["size"], c["p"], None)
    finally:
        head_concat.draw_keep = orig
    N, (OH, OW) = maps[0].shape[0], c["size"]
    assert [tuple(k.shape) for _, k in drawn] == [(N, OH, OW, m.shape[1]) for m, q in zip(maps, c["p"]) if q is not None]
    for p, k in drawn:
        n, kept = k.numel(), int(k.sum())
        assert k.dtype == torch.uint8 and int(k.max()) == 1 and p == hc.P
        sigma = math.sqrt(p * (1 - p) / n)
        print(f"drawn mask of {n} elements: kept {kept / n:.5f}, 1 - p = {1 - p}, {abs(kept / n - (1 - p)) / sigma:.2f} sigma")
        assert abs(kept / n - (1 - p)) <= 6 * sigma
    k0 = drawn[0][1]                                                                   # the op applied what it drew
    assert bool((y[:, :maps[0].shape[1]][k0.permute(0, 3, 1, 2) == 0] == 0).all())


CHILD = r"""
import sys
import torch
sys.path.insert(0, "tests")
import head_concat_cases as hc
from vivim_amd import _lib
from vivim_amd.head_concat import upsample_concat
assert _lib.GUARD
dev = torch.device("cuda:0")
n = 0
for name, dt, masks in (("ratios", "bf16", "some"), ("ratios", "fp32", "all"), ("odd_c", "fp16", "some"), ("odd_c", "fp32", "none"),
                        ("one_map", "bf16", "all"), ("wide", "bf16", "some"), ("wide", "fp32", "all"), ("c768", "bf16", "some")):
    c = hc.case(name, dt, masks)
    maps = [m.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True) for m in c["maps"]]
    keep = [None if k is None else k.to(dev) for k in c["keep"]]
    y = upsample_concat(maps, c["size"], c["p"], keep)
    y.backward(c["go"].to(dev).contiguous(memory_format=torch.channels_last))
    _lib.check_guards("head_concat")
    assert torch.isfinite(y.float()).all() and all(torch.isfinite(m.grad.float()).all() for m in maps)
    n += 1
print("GUARD_OK", n)
"""


def test_writes_stay_inside_out_and_dmaps_under_guard(cuda):
    env = dict(os.environ, VIVIM_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GUARD_OK 8" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---- the head inside Vivim ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def head(cuda):
    h = hc.build_head(cuda)
    on_cpu = {k: hc.to_device(v, "cpu") for k, v in h.items() if k != "model"}      # the fp64 copy runs on the CPU and replays the masks:
    ref = copy.deepcopy(h["model"]).double().cpu()                                   # computed once, shared
    want = hc.run_head(on_cpu, ref, False, double=True)
    h["want"] = (want[0].to(cuda), {n: g.to(cuda) for n, g in want[1].items()}, want[2], want[3])
    return h


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_head_in_vivim_against_fp64(dt, head):
    model, amp = head["model"], (torch.bfloat16 if dt == "bf16" else None)
    expected = amp or torch.float32
    assert head["want"][3] == {"draw_keep": 0, "F.dropout": 4} and head["want"][2].dtype == torch.float64
    new, names_new = _calls(lambda: hc.run_head(head, model, True, autocast=amp))
    stock, names_stock = _calls(lambda: hc.run_head(head, model, False, autocast=amp))
    # which route ran, and on which masks
    assert names_new.count("vivim_head_concat_fwd") == 1 and names_new.count("vivim_head_concat_bwd") == 1
    assert not [n for n in names_stock if n.startswith("vivim_head_concat")]
    assert new[3] == {"draw_keep": 4, "F.dropout": 0} and stock[3] == {"draw_keep": 0, "F.dropout": 4}
    # what linear_fuse was handed
    concat = new[2]
    assert concat.dtype == expected and concat.shape == (4, 4 * 768, 16, 16) and concat.is_contiguous(memory_format=torch.channels_last)
    assert stock[2].dtype == torch.float32                                            # the stock route's fp32 concat, autocast or not
    assert torch.isfinite(new[0].float()).all() and all(torch.isfinite(g.float()).all() for g in new[1].values())
    e_new, e_stock = hc.head_errors(new[:2], head["want"][:2]), hc.head_errors(stock[:2], head["want"][:2])
    failed = []
    for n in e_new:
        (en, scale), (es, _) = e_new[n], e_stock[n]
        print(f"head in Vivim [{dt}] {n}: err new {en:.3e}, stock {es:.3e}, max|want| {scale:.3e}, allowed {2 * es + hc.FLOOR * scale:.3e}")
        _log(f"head_in_vivim[{dt}]", n, expected, en / (2 * es + hc.FLOOR * scale))
        if not en <= 2 * es + hc.FLOOR * scale:
            failed.append(n)
    assert not failed, failed


def test_no_mask_is_drawn_where_the_coin_says_no_or_in_eval_mode(cuda):
    from vivim_amd import head_concat
    h = hc.build_head(cuda, seed=hc.MIXED_SEED)
    model, drawn, orig = h["model"], [], head_concat.draw_keep
    head_concat.draw_keep = lambda shape, p, device: drawn.append((tuple(shape), p)) or orig(shape, p, device)
    try:
        for train in (True, False):
            model.train(train)
            del drawn[:]
            torch.manual_seed(hc.MIXED_SEED)
            out, names = _calls(lambda: model.decode(h["states"], 1, 4))
            assert names.count("vivim_head_concat_fwd") == 1 and torch.isfinite(out).all()
            after = torch.get_rng_state()
            assert drawn == ([((4, 16, 16, 768), h["p"])] * sum(h["coins"]) if train else [])
            model.fused_head_concat = False
            try:
                torch.manual_seed(hc.MIXED_SEED)
                model.decode(h["states"], 1, 4)
                assert torch.equal(after, torch.get_rng_state())                       # the same coins were flipped on the CPU
            finally:
                model.fused_head_concat = True
    finally:
        head_concat.draw_keep = orig
