"""CPU: the training decode head's concat op below the GPU.  The extension header include/vivim_hip_ext_head.h parses into its row
of _lib.EXTENSIONS (what the registry as a whole holds: test_abi_extensions.py); the struct's layout is the C compiler's; every
host-side refusal of the two entry points, with its message, directly and through _lib.call; `supported` on CPU and meta tensors;
the switch's keyword; on the CPU the switch changes neither a bit nor the RNG state; the stock composition against the fp64
reference; and the kernels' arithmetic restated in torch fp32 (head_concat_cases.restate32) held to the GPU test's bounds on the GPU
test's inputs."""
import ctypes
import inspect
import os

import pytest
import torch

import head_concat_cases as hc
from abi_cases import PTR, layout_matches_c, refused as _refused
from conftest import ROOT
from test_gpu_upsample import RHO
from vivim_amd import _lib
from vivim_amd import head_concat

HEAD_HEADER = os.path.join(ROOT, "include", "vivim_hip_ext_head.h")
NAMES = ("vivim_head_concat_fwd", "vivim_head_concat_bwd")
STRUCTURE_LOSS = ("vivim_structure_loss_workspace_bytes", "vivim_structure_loss_fwd", "vivim_structure_loss_bwd")
BINARY_METRICS = ("vivim_binary_metrics_workspace_bytes", "vivim_binary_metrics")
P = _lib.HeadConcatParams
FIELDS = ["struct_bytes", "batch", "n_maps", "out_h", "out_w", "itype", "map_c", "map_h", "map_w", "chan_off", "scale",
          "map_batch_stride", "dmap_batch_stride", "keep_batch_stride", "out_batch_stride", "out_pixel_stride", "maps", "keep", "out",
          "dout", "dmaps"]


# ---- the header and the tables

def test_the_header_parses_into_its_own_table():
    names, entries = _lib.EXTENSIONS["vivim_hip_ext_head.h"]
    assert names == {"vivim_head_concat_params": "HeadConcatParams"} and tuple(entries) == NAMES
    consts, classes, parsed = _lib.parse_header(open(HEAD_HEADER).read(), names)
    assert consts == {} and list(classes) == ["HeadConcatParams"] and tuple(parsed) == NAMES
    ptr = ctypes.POINTER(P)
    assert entries == {n: _lib.Entry(None, (ptr,), True, ctypes.c_int) for n in NAMES}
    assert [n for n, _ in P._fields_] == FIELDS and ctypes.sizeof(P) == 328
    types = dict(P._fields_)
    assert types["scale"] is ctypes.c_float * 4 and types["map_c"] is ctypes.c_int32 * 4 and types["keep"] is ctypes.c_void_p * 4
    assert types["keep_batch_stride"] is ctypes.c_int64 * 4 and types["out_pixel_stride"] is ctypes.c_int64
    text = open(HEAD_HEADER).read()
    assert "#ifndef VIVIM_HIP_EXT_HEAD_H" in text and '#include "vivim_hip.h"' in text
    assert list(_lib.EXTENSIONS) == ["vivim_hip_ext.h", "vivim_hip_ext_head.h", "vivim_hip_ext_binary_metrics.h"]
    assert set(_lib.ALL_ENTRY_POINTS) == set(_lib.ENTRY_POINTS) | set(STRUCTURE_LOSS) | set(NAMES) | set(BINARY_METRICS)
    assert len(_lib.ALL_ENTRY_POINTS) == 60


def test_the_parser_admits_the_new_guard_and_nothing_else():
    ok = "#ifndef VIVIM_HIP_EXT_HEAD_H\n#define VIVIM_HIP_EXT_HEAD_H\nint vivim_x(void);\n#endif\n"
    assert list(_lib.parse_header(ok, {})[2]) == ["vivim_x"]
    for bad in ("#ifndef VIVIM_HIP_ext_H", "#ifndef VIVIM_HIPEXT_H", "#ifndef OTHER_H", "#ifndef VIVIM_HIP_EXT_", "#if 1", "#pragma once",
                "#ifndef VIVIM_HIP__H"):
        with pytest.raises(ValueError, match="a preprocessor line it does not know"):
            _lib.parse_header(bad + "\nint vivim_x(void);\n#endif\n", {})


def test_the_library_exports_the_two_symbols():
    L = _lib.lib()
    for n in NAMES:
        fn = getattr(L, n)
        assert fn.argtypes == [ctypes.POINTER(P), ctypes.c_void_p] and fn.restype is ctypes.c_int


def test_layout_matches_the_c_compiler(tmp_path):
    layout_matches_c("vivim_hip_ext_head.h", "vivim_head_concat_params", P, tmp_path)


# ---- refusals

def _good(**over):
    """Two bf16 maps (8, 2, 3) and (16, 4, 6) of 2 images into (4, 6) with a pixel stride of 24; `name=(index, value)` sets one
    array element, `name=value` a whole field."""
    p = P()
    p.struct_bytes = ctypes.sizeof(P)
    p.batch, p.n_maps, p.out_h, p.out_w, p.itype = 2, 2, 4, 6, _lib.BF16
    for s, (c, h, w, off) in enumerate(((8, 2, 3, 0), (16, 4, 6, 8))):
        p.map_c[s], p.map_h[s], p.map_w[s], p.chan_off[s], p.scale[s] = c, h, w, off, 1.0
        p.map_batch_stride[s] = p.dmap_batch_stride[s] = c * h * w
        p.keep_batch_stride[s] = c * 4 * 6
        p.maps[s] = p.keep[s] = p.dmaps[s] = PTR
    p.out_batch_stride, p.out_pixel_stride = 4 * 6 * 24, 24
    p.out = p.dout = PTR
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


@pytest.mark.parametrize("name", NAMES)
def test_refusals_before_any_launch(name):
    fn, bwd = name[len("vivim_"):], name.endswith("bwd")
    assert f"{fn}: params is NULL" in _refused(name, None)
    assert "struct_bytes = 0, this library's vivim_head_concat_params has 328" in _refused(name, _good(struct_bytes=0))
    assert "struct_bytes = 336" in _refused(name, _good(struct_bytes=336))
    for v in (0, 5, -1):
        assert f"n_maps = {v}: one to four maps" in _refused(name, _good(n_maps=v))
    assert "itype = 7" in _refused(name, _good(itype=7))
    for field in ("batch", "out_h", "out_w"):
        for v in (0, -3):
            assert f"{field} = {v}" in _refused(name, _good(**{field: v})), field
    for field in ("map_c", "map_h", "map_w"):
        for v in (0, -3):
            assert f"map 1: " in _refused(name, _good(**{field: (1, v)})) and f"{field} = {v}" in _refused(name, _good(**{field: (1, v)}))
    assert "map 0 is (5, 3), the output (4, 6): upsampling only" in _refused(name, _good(map_h=(0, 5)), code=2)
    assert "map 1 is (4, 7), the output (4, 6): upsampling only" in _refused(name, _good(map_w=(1, 7)), code=2)
    assert "map 1: channels [9, 25) lie outside a pixel of out_pixel_stride = 24" in _refused(name, _good(chan_off=(1, 9)))
    assert "map 0: channels [-1, 7) lie outside" in _refused(name, _good(chan_off=(0, -1)))
    assert "the channel blocks of maps 0 and 1 overlap: [0, 8) and [7, 23)" in _refused(name, _good(chan_off=(1, 7)))
    assert "the channel blocks of maps 0 and 1 overlap: [8, 16) and [8, 24)" in _refused(name, _good(chan_off=(0, 8)))
    big, small = ("dout", "dmaps") if bwd else ("out", "maps")
    assert f"{big} at (nil)" in _refused(name, _good(**{big: None}))
    assert f"{big} at 0x1001: need a 2-byte aligned pointer" in _refused(name, _good(**{big: PTR + 1}))
    assert f"{small}[1] at (nil)" in _refused(name, _good(**{small: (1, None)}))
    assert f"{small}[0] at 0x1001: need a 2-byte aligned pointer" in _refused(name, _good(**{small: (0, PTR + 1)}))
    assert f"{small}[0] at 0x1002: need a 4-byte aligned pointer" in _refused(name, _good(itype=_lib.F32, **{small: (0, PTR + 2)}))
    for v, text in ((0.5, "0.5"), (float("inf"), "inf"), (float("nan"), "nan"), (-2.0, "-2")):
        assert f"scale[1] = {text}: 1 / (1 - p) is finite and at least 1" in _refused(name, _good(scale=(1, v)))
    assert "out_batch_stride = 575: an image of out has 576 elements" in _refused(name, _good(out_batch_stride=575))
    stride = "dmap_batch_stride" if bwd else "map_batch_stride"
    assert f"{stride}[1] = 383: an image of map 1 has 384 elements" in _refused(name, _good(**{stride: (1, 383)}))
    assert "keep_batch_stride[0] = 191: a mask of map 0 has 192 bytes" in _refused(name, _good(keep_batch_stride=(0, 191)))
    for over in (dict(out_h=1 << 15, out_w=1 << 15),                               # an image of out past 2^31 elements
                 dict(batch=1 << 20, out_h=1 << 12),                               # batch * out_h
                 dict(out_h=1 << 16, map_h=(1, 1 << 15)),                          # (2 H + 3) OH: the window arithmetic
                 dict(out_w=1 << 16, map_w=(1, 1 << 15)),
                 dict(batch=1 << 20, out_h=1 << 10, out_w=1 << 10, map_h=(1, 1 << 10), map_w=(1, 1 << 10))):     # the grid, either direction
        assert "the index range overflows int32" in _refused(name, _roomy(**over)), over


def _roomy(**over):
    """_good without masks and with batch strides that any size fits: what only the index-range check can refuse."""
    p = _good(out_batch_stride=1 << 62, **over)
    for s in range(2):
        p.keep[s], p.map_batch_stride[s], p.dmap_batch_stride[s] = None, 1 << 40, 1 << 40
    return p


def test_a_missing_mask_or_unused_slots_are_not_refused_by_the_checks_before_them():
    """keep[s] NULL is "no mask", and slots at and beyond n_maps are not read: bad values there change no verdict."""
    p = _good(struct_bytes=0, keep=(0, None))
    p.map_c[3], p.scale[2] = -1, float("nan")
    assert "struct_bytes = 0" in _refused(NAMES[0], p)
    q = _good(out=None, dout=None)
    q.map_c[3], q.scale[2], q.keep[1] = -1, float("nan"), None
    for name in NAMES:
        assert "at (nil)" in _refused(name, q)                       # the first check a good two-map struct with bad unused slots fails


# ---- gating

def test_supported_says_no_off_the_gpu_and_the_op_is_the_stock_composition():
    c = hc.case("odd_c", "fp32", "some")
    maps = [m.contiguous(memory_format=torch.channels_last) for m in c["maps"]]
    assert not head_concat.supported(maps, c["size"]) and not head_concat.supported(maps, c["size"], c["keep"])
    assert not head_concat.supported([m.to("meta") for m in maps], c["size"])
    assert not head_concat.supported([], c["size"]) and not head_concat.supported(maps * 2, c["size"])
    assert not head_concat.supported(maps[0], c["size"]) and not head_concat.supported(maps, (7,))
    with pytest.raises(ValueError, match="one probability"):
        head_concat.upsample_concat(maps, c["size"], p=[0.1])
    with pytest.raises(ValueError, match="one probability"):
        head_concat.upsample_concat(maps, c["size"], p=[0.1, 1.0, None])
    with pytest.raises(ValueError, match="2 masks for 3 maps"):
        head_concat.upsample_concat(maps, c["size"], keep=c["keep"][:2])


@pytest.mark.parametrize("name,dt", [("odd_c", "fp32"), ("ratios", "fp32"), ("ratios", "bf16"), ("one_map", "fp32")])
def test_the_stock_composition_against_the_fp64_reference(name, dt):
    """CPU tensors: upsample_concat is F.interpolate, times mask and scale, torch.cat.  ATen's forward is held to twice the bound,
    as test_gpu_upsample.py holds it; in a 16-bit type the composition rounds twice (the upsampled value, then the product), so one
    more rho |want| is allowed there.  The fp32 gradient through autograd likewise."""
    c = hc.case(name, dt, "some")
    maps = [m.clone().requires_grad_(True) for m in c["maps"]]
    y = head_concat.upsample_concat(maps, c["size"], c["p"], c["keep"])
    assert y.dtype == c["dtype"] and y.shape == c["go"].shape
    if dt == "fp32":
        y.backward(c["go"])
    for s, r in enumerate(c["refs"]):
        C = maps[s].shape[1]
        ey = (y[:, r["off"]:r["off"] + C].detach().double() - r["want"]).abs()
        hc.within(ey, 2 * r["fwd_bound"] + RHO[c["dtype"]] * r["want"].abs(), f"stock y of map {s}")
        if dt == "fp32":
            hc.within((maps[s].grad.double() - r["want_b"]).abs(), 2 * r["bwd_bound"], f"stock dx of map {s}")
        if c["keep"][s] is not None:
            dropped = c["keep"][s].permute(0, 3, 1, 2) == 0
            assert bool((y[:, r["off"]:r["off"] + C][dropped] == 0).all())
    drawn = []
    orig = head_concat.draw_keep
    head_concat.draw_keep = lambda shape, p, device: drawn.append((tuple(shape), p)) or torch.ones(shape, dtype=torch.uint8)
    try:
        head_concat.upsample_concat(c["maps"], c["size"], c["p"])
    finally:
        head_concat.draw_keep = orig
    N, (OH, OW) = c["maps"][0].shape[0], c["size"]
    assert drawn == [((N, OH, OW, m.shape[1]), hc.P) for m, q in zip(c["maps"], c["p"]) if q is not None]


# ---- the kernels' arithmetic, restated in fp32

RESTATE_WORST = {}


@pytest.mark.parametrize("name,dt,masks", hc.GRID)
def test_restated_arithmetic_meets_the_gpu_bounds(name, dt, masks):
    """Every case of tests/test_gpu_head_concat.py's grid through head_concat_cases.restate32 and the same bounds: they are
    reachable by fp32 arithmetic of the kernels' form.  Prints the worst error as a share of its bound."""
    c = hc.case(name, dt, masks)
    y, dxs = hc.restate32(c["maps"], c["go"], c["keep"], [r["scale"] for r in c["refs"]], c["size"], c["dtype"])
    wf, wb = hc.check(c, y, dxs, f"restate32[{name} {dt} {masks}]")
    RESTATE_WORST[(name, dt, masks)] = (wf, wb)
    print(f"restate32[{name} {dt} {masks}]: worst err / bound forward {wf:.3f}, backward {wb:.3f}")
    assert wf <= 1.0 and wb <= 1.0
    for s, k in enumerate(c["keep"]):
        if k is not None:
            r, C = c["refs"][s], c["maps"][s].shape[1]
            assert bool((y[:, r["off"]:r["off"] + C][k.permute(0, 3, 1, 2) == 0] == 0).all())


# ---- the switch

def test_the_switch_is_the_last_keyword_and_off():
    from vivim_amd import train_step, vivim
    for fn in (vivim.Vivim.__init__, train_step.build_model):
        params = inspect.signature(fn).parameters
        assert list(params)[-1] == "fused_head_concat" and params["fused_head_concat"].default is False
    assert list(inspect.signature(vivim.Vivim.__init__).parameters)[-2] == "fused_backbone_add_norm"
    assert list(inspect.signature(train_step.build_model).parameters)[-2] == "low_precision_params"
    sig = inspect.signature(head_concat.upsample_concat).parameters
    assert list(sig) == ["maps", "size", "p", "keep"] and sig["p"].default is None and sig["keep"].default is None


def _cpu_head():
    from transformers import SegformerConfig, SegformerForSemanticSegmentation
    from vivim_amd.vivim import Vivim
    torch.manual_seed(3)
    cfg = SegformerConfig(num_channels=3, num_encoder_blocks=4, depths=[1, 1, 1, 1], sr_ratios=[8, 4, 2, 1],
                          hidden_sizes=[16, 24, 40, 64], patch_sizes=[7, 3, 3, 3], strides=[4, 2, 2, 2],
                          num_attention_heads=[1, 2, 5, 8], mlp_ratios=[2, 2, 2, 2], decoder_hidden_size=768, num_labels=4)
    model = Vivim(in_chans=3, out_chans=3, depths=[1, 1, 1, 1], feat_size=[16, 24, 40, 64], backbone=SegformerForSemanticSegmentation(cfg),
                  fused_head_concat=True)
    g = torch.Generator().manual_seed(4)
    states = tuple(torch.randn(2, c, s, s, generator=g) for c, s in zip((16, 24, 40, 64), (8, 4, 2, 1)))
    return model, states


@pytest.mark.parametrize("train", [True, False])
def test_on_the_cpu_the_switch_changes_neither_a_bit_nor_the_rng_state(train, monkeypatch):
    model, states = _cpu_head()
    model.train(train)
    assert model.fused_head_concat
    out = {}
    for switch in (True, False, "env"):
        model.fused_head_concat = bool(switch)
        if switch == "env":
            monkeypatch.setenv("VIVIM_NO_HEAD_CONCAT", "1")
        torch.manual_seed(17)
        model.zero_grad(set_to_none=True)
        y = model.decode(states, 1, 2)
        y.sum().backward()
        out[switch] = (y.detach(), torch.get_rng_state(), [p.grad.clone() for p in model.parameters() if p.grad is not None])
    for other in (False, "env"):
        assert torch.equal(out[True][0], out[other][0]) and torch.equal(out[True][1], out[other][1])
        assert len(out[True][2]) == len(out[other][2]) > 8
        assert all(torch.equal(a, b) for a, b in zip(out[True][2], out[other][2]))


def test_the_fp32_head_on_the_cpu_sets_the_floor():
    """head_concat_cases.FLOOR, the allowance of tests/test_gpu_head_concat.py's comparison inside Vivim, is 4 x the worst error of
    the fp32 head on the CPU against the fp64 head on the same states and masks."""
    import copy
    h = hc.build_head("cpu")
    want = hc.run_head(h, copy.deepcopy(h["model"]).double(), False, double=True)
    got = hc.run_head(h, h["model"], True)
    assert got[3] == want[3] == {"draw_keep": 0, "F.dropout": 4}                  # CPU tensors: the stock path, every coin says yes
    errs = hc.head_errors(got[:2], want[:2])
    name, worst = max(((n, e / m) for n, (e, m) in errs.items()), key=lambda t: t[1])
    print(f"fp32 head on the CPU against fp64: worst max|err| / max|want| {worst:.3e} ({name}); floor {hc.FLOOR:.1e}")
    assert 4 * worst <= hc.FLOOR
