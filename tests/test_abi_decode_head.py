"""CPU: the fused decode head's entry point (include/vivim_hip.h: vivim_decode_head_params) is declared, exported and present
without disturbing the binding's tables; every bad argument is refused on the host before any launch; the fold
(vivim_amd.fold_decode_head) reproduces the stock eval-mode head; and on CPU tensors, in train mode or with grad enabled the
switch changes nothing."""
import copy
import ctypes
import functools
import inspect
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import ROOT
from vivim_amd import _lib

NAME = "vivim_decode_head_fwd"
OK, INVALID, UNSUPPORTED = 0, 1, 2
PTR = 1 << 20                                    # a non-null, 16-byte aligned address: no check may dereference it
MAX_HIDDEN = 1024
POINTERS = ("maps0", "maps1", "maps2", "maps3", "bias", "w_out", "logits")


def _params(N=2, K=16, C=3, OH=16, OW=16, maps=((16, 16), (8, 8), (4, 4), (2, 2)), itype=_lib.F32):
    P = _lib.DecodeHeadParams()
    P.struct_bytes = ctypes.sizeof(_lib.DecodeHeadParams)
    P.batch, P.hidden, P.classes, P.n_maps, P.out_h, P.out_w, P.itype = N, K, C, len(maps), OH, OW, itype
    for s, (h, w) in enumerate(maps):
        P.map_h[s], P.map_w[s], P.map_batch_stride[s], P.maps[s] = h, w, K * h * w, PTR
    P.logits_batch_stride = C * OH * OW
    P.bias = P.w_out = P.b_out = P.logits = PTR
    return P


def _set(P, field, value):
    """setattr that also reaches one element of an array field: "map_h2" is map_h[2]."""
    m = re.fullmatch(r"(maps|map_h|map_w|map_batch_stride)(\d)", field)
    if m:
        getattr(P, m.group(1))[int(m.group(2))] = value
    else:
        setattr(P, field, value)


def _refused(P, code, message=None):
    """`code` and nothing launched: the pointers are not memory, so a kernel that started would not return an error code."""
    L = _lib.lib()
    assert L.vivim_decode_head_fwd(ctypes.byref(P), None) == code, L.vivim_last_error()
    assert L.vivim_last_error() != b""
    if message is not None:
        assert message in L.vivim_last_error(), L.vivim_last_error()
    return L.vivim_last_error()


def test_symbol_declared_exported_and_present():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vivim_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vivim_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    assert NAME in declared and NAME in _lib.EXPORTS and hasattr(L, NAME)
    assert getattr(L, NAME).argtypes == [ctypes.POINTER(_lib.DecodeHeadParams), ctypes.c_void_p]
    assert "vivim_decode_head_params" in text


def test_the_tables_are_undisturbed():
    """No vivim_sizeof row, not in STRUCTS, struct None in the entry-point table, ABI version unchanged."""
    L = _lib.lib()
    e = _lib.ENTRY_POINTS[NAME]
    assert e.struct is None and e.extra == (ctypes.POINTER(_lib.DecodeHeadParams),) and e.stream and e.restype is ctypes.c_int
    assert len(_lib.STRUCTS) == 15 and _lib.DecodeHeadParams not in _lib.STRUCTS
    assert L.vivim_sizeof(15) == 0
    assert L.vivim_abi_version() == 8
    names = [f[0] for f in _lib.DecodeHeadParams._fields_]
    assert names == ["struct_bytes", "batch", "hidden", "classes", "n_maps", "out_h", "out_w", "itype", "map_h", "map_w",
                     "map_batch_stride", "logits_batch_stride", "maps", "bias", "w_out", "b_out", "logits"]


def test_null_struct_and_struct_bytes():
    L = _lib.lib()
    assert L.vivim_decode_head_fwd(None, None) == INVALID and b"check failed" in L.vivim_last_error()
    size = ctypes.sizeof(_lib.DecodeHeadParams)
    for off in (-1, 1):
        P = _params()
        P.struct_bytes = size + off
        _refused(P, INVALID, b"struct_bytes = %d" % (size + off))
    P = _params()
    P.struct_bytes = 0
    _refused(P, INVALID, b"struct_bytes")


def test_call_and_launch_reach_it():
    """_lib.call passes byref(params) first: the refusal text comes back as a RuntimeError."""
    P = _params()
    P.struct_bytes -= 1
    with pytest.raises(RuntimeError, match="struct_bytes"):
        _lib.call(NAME, P, 0)


def test_bad_sizes_counts_and_types():
    for field in ("batch", "hidden", "classes", "out_h", "out_w", "map_h0", "map_w1", "map_h3", "map_w3"):
        for v in (0, -1):
            P = _params()
            _set(P, field, v)
            _refused(P, INVALID, b"check failed")
    for field, v in (("n_maps", 0), ("n_maps", 5), ("n_maps", -1), ("classes", 9), ("itype", 3), ("itype", -1)):
        P = _params()
        _set(P, field, v)
        _refused(P, INVALID, b"check failed")
    P = _params(K=MAX_HIDDEN + 1)
    _refused(P, INVALID, b"hidden = %d" % (MAX_HIDDEN + 1))
    # an unused map slot is not looked at
    P = _params(maps=((16, 16), (8, 8)))
    P.map_h[3] = -5
    P.maps[2] = None
    P.b_out = None
    P.logits_batch_stride = 1
    _refused(P, INVALID, b"logits_batch_stride")


def test_null_pointers():
    for field in POINTERS:
        P = _params()
        _set(P, field, None)
        _refused(P, INVALID, b"check failed")
    # b_out may be NULL: the call gets as far as the next check, the batch strides
    P = _params()
    P.b_out = None
    P.map_batch_stride[1] -= 1
    _refused(P, INVALID, b"map_batch_stride")


def test_misaligned_pointers():
    for itype, offs in ((_lib.F32, (1, 2)), (_lib.F16, (1,)), (_lib.BF16, (1,))):
        for off in offs:
            for field in POINTERS + ("b_out",):
                P = _params(itype=itype)
                _set(P, field, PTR + off)
                _refused(P, INVALID, b"check failed")
    for field in ("bias", "w_out", "b_out"):                 # fp32 whatever the maps' type
        P = _params(itype=_lib.BF16)
        _set(P, field, PTR + 2)
        _refused(P, INVALID, b"check failed")
    P = _params(itype=_lib.BF16)                            # two bytes off is element-aligned for a 16-bit map
    P.maps[1] = PTR + 2
    P.logits_batch_stride -= 1
    _refused(P, INVALID, b"logits_batch_stride")


def test_batch_strides_smaller_than_an_image():
    for s in range(4):
        P = _params()
        P.map_batch_stride[s] -= 1
        _refused(P, INVALID, b"map_batch_stride")
    P = _params()
    P.logits_batch_stride -= 1
    _refused(P, INVALID, b"logits_batch_stride")
    P = _params(N=1)                                        # also for a single image
    P.map_batch_stride[0] = 0
    _refused(P, INVALID, b"map_batch_stride")


def test_sizes_past_31_bits_are_refused():
    big = 1 << 11
    for kw in (dict(K=1024, OH=big, OW=big, maps=((big, big),)),                 # one map image of 2^32 elements
               dict(K=8, C=8, OH=1 << 14, OW=1 << 14, maps=((1, 1),)),           # one logits image of 2^31 elements
               dict(N=1 << 21, K=8, OH=256, OW=256, maps=((1, 1),))):            # 2^21 images of 32 x 32 tiles: 2^31 workgroups
        P = _params(**kw)
        P.map_batch_stride[0] = P.logits_batch_stride = 1 << 40
        _refused(P, INVALID, b"check failed")


def test_a_map_larger_than_the_output_is_unsupported_with_a_message():
    for maps in (((17, 16),), ((16, 17),), ((16, 16), (8, 8), (4, 32), (2, 2)), ((16, 16), (8, 8), (4, 4), (40, 40))):
        _refused(_params(maps=maps), UNSUPPORTED, b"upsampling only")


def test_algorithmic_bytes_has_a_branch_for_the_new_name():
    P = _params(N=2, K=16, C=3, OH=16, OW=16, itype=_lib.BF16)
    maps_px = 256 + 64 + 16 + 4
    assert _lib.algorithmic_bytes(NAME, P) == 2 * (maps_px * 16 + 3 * 256) * 2 + 4 * (16 + 3 * 16 + 3)
    P = _params(N=1, K=8, C=2, OH=4, OW=6, maps=((4, 6), (2, 3)), itype=_lib.F32)
    assert _lib.algorithmic_bytes(NAME, P) == (30 * 8 + 2 * 24) * 4 + 4 * (8 + 2 * 8 + 2)


def test_exported_from_the_package_and_off_by_default():
    import vivim_amd
    from vivim_amd import decode_head, train_step, vivim
    assert vivim_amd.fused_decode_head is decode_head.fused_decode_head
    assert vivim_amd.fold_decode_head is decode_head.fold_decode_head
    assert inspect.signature(vivim.Vivim.__init__).parameters["fused_decode_head"].default is False
    assert inspect.signature(train_step.build_model).parameters["fused_decode_head"].default is False
    assert decode_head.MAX_HIDDEN == MAX_HIDDEN


def test_supported_is_false_for_cpu_tensors():
    from vivim_amd import decode_head
    maps = [torch.randn(2, 4, 4, 16), torch.randn(2, 2, 2, 16)]
    assert decode_head.supported(maps, torch.randn(16), torch.randn(3, 16), torch.randn(3), (4, 4)) is False
    with pytest.raises(RuntimeError, match="unsupported"):
        decode_head.fused_decode_head(maps, torch.randn(16), torch.randn(3, 16), None, (4, 4))


# ---- the fold -------------------------------------------------------------------------------------------------------------------
DIMS = (64, 128, 320, 512)


def _randomise_head(decoder, seed):
    """BatchNorm statistics and affine, and the projection biases, away from their initial values."""
    from vivim_amd.decode_head import _projections
    g = torch.Generator().manual_seed(seed)
    bn = decoder.batch_norm
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(bn.num_features, generator=g))
        bn.running_var.copy_(torch.rand(bn.num_features, generator=g) * 1.5 + 0.5)
        bn.weight.copy_(torch.randn(bn.num_features, generator=g))
        bn.bias.copy_(torch.randn(bn.num_features, generator=g))
        for proj in _projections(decoder):
            proj.bias.copy_(torch.randn(proj.out_features, generator=g))


def _stock_eval_head(decoder, out_conv, states):
    """The eval-mode head as Vivim.decode computes it (dropouts are identities), in the modules' own dtype."""
    from vivim_amd.decode_head import _projections
    size0, feats = states[0].shape[2:], ()
    for x, proj in zip(states, _projections(decoder)):
        t = proj(x.flatten(2).transpose(1, 2)).permute(0, 2, 1).reshape(x.shape[0], -1, *x.shape[2:])
        feats += (F.interpolate(t, size=size0, mode="bilinear", align_corners=False),)
    hidden = decoder.activation(decoder.batch_norm(decoder.linear_fuse(torch.cat(feats[::-1], dim=1))))
    return out_conv(hidden)


def _folded_with_torch_ops(fold, states):
    weights, bias, w_out, b_out = fold
    size0, total = states[0].shape[2:], 0
    for x, w in zip(states, weights):
        m = F.linear(x.flatten(2).transpose(1, 2), w).view(x.shape[0], x.shape[2], x.shape[3], -1).permute(0, 3, 1, 2)
        total = total + F.interpolate(m, size=size0, mode="bilinear", align_corners=False)
    return F.conv2d(F.relu(total + bias[None, :, None, None]), w_out[:, :, None, None], b_out)


@functools.lru_cache(maxsize=None)
def _head():
    from transformers import SegformerConfig
    from transformers.models.segformer.modeling_segformer import SegformerDecodeHead
    torch.manual_seed(21)
    cfg = SegformerConfig(num_encoder_blocks=4, hidden_sizes=list(DIMS), decoder_hidden_size=768, num_labels=150)
    decoder, out_conv = SegformerDecodeHead(cfg).eval(), nn.Conv2d(768, 3, 1)
    _randomise_head(decoder, 22)
    return decoder, out_conv, copy.deepcopy(decoder).double(), copy.deepcopy(out_conv).double()


def _rel(got, want):
    return float((got.double() - want).norm() / want.norm())


@pytest.mark.parametrize("N,sizes", [(2, ((16, 16), (8, 8), (4, 4), (2, 2))), (1, ((8, 12), (4, 6), (2, 3), (1, 2)))])
def test_fold_reproduces_the_stock_eval_head(N, sizes):
    """Norm-wise < 1e-5 against an fp64 evaluation of the stock head (both sides fp32: the project's 1e-3 bar tightened by two
    orders); with the stage blocks of linear_fuse taken in ascending order instead of feats[::-1] the same bound is missed."""
    from vivim_amd import fold_decode_head
    decoder, out_conv, decoder64, out64 = _head()
    g = torch.Generator().manual_seed(23 + N)
    states = [torch.randn(N, c, h, w, generator=g) for c, (h, w) in zip(DIMS, sizes)]
    with torch.no_grad():
        want = _stock_eval_head(decoder64, out64, [x.double() for x in states])
        fold = fold_decode_head(decoder, out_conv)
        assert all(t.dtype == torch.float32 for t in list(fold[0]) + list(fold[1:]))
        assert [tuple(w.shape) for w in fold[0]] == [(768, c) for c in DIMS] and fold[1].shape == (768,) and fold[2].shape == (3, 768)
        err = _rel(_folded_with_torch_ops(fold, states), want)
        # block(s) = s: the fold of a head whose linear_fuse has its four column blocks in the opposite order
        swapped = copy.deepcopy(decoder)
        blocks = decoder.linear_fuse.weight.split(768, dim=1)
        swapped.linear_fuse.weight.copy_(torch.cat(blocks[::-1], dim=1))
        err_swapped = _rel(_folded_with_torch_ops(fold_decode_head(swapped, out_conv), states), want)
    print(f"fold against the fp64 stock head: {err:.3e}; with block(s) = s: {err_swapped:.3e}")
    assert err < 1e-5
    assert not err_swapped < 1e-5


def test_fold_takes_a_linear_fuse_bias_and_a_head_without_out_bias():
    decoder, out_conv, _, _ = _head()
    decoder, out_conv = copy.deepcopy(decoder), nn.Conv2d(768, 2, 1, bias=False)
    fuse = nn.Conv2d(4 * 768, 768, 1, bias=True)
    with torch.no_grad():
        fuse.weight.copy_(decoder.linear_fuse.weight)
        fuse.bias.normal_()
    decoder.linear_fuse = fuse
    from vivim_amd import fold_decode_head
    g = torch.Generator().manual_seed(29)
    states = [torch.randn(1, c, h, h, generator=g) for c, h in zip(DIMS, (8, 4, 2, 1))]
    with torch.no_grad():
        want = _stock_eval_head(copy.deepcopy(decoder).double(), copy.deepcopy(out_conv).double(), [x.double() for x in states])
        fold = fold_decode_head(decoder, out_conv)
        assert fold[3] is None
        assert _rel(_folded_with_torch_ops(fold, states), want) < 1e-5


# ---- the switch -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _models():
    """Two Vivims with equal weights on a depth-1 backbone, the switch on and off."""
    from transformers import SegformerConfig, SegformerForSemanticSegmentation
    from vivim_amd.vivim import Vivim
    cfg = SegformerConfig(num_channels=3, num_encoder_blocks=4, depths=[1, 1, 1, 1], sr_ratios=[8, 4, 2, 1],
                          hidden_sizes=list(DIMS), patch_sizes=[7, 3, 3, 3], strides=[4, 2, 2, 2],
                          num_attention_heads=[1, 2, 5, 8], mlp_ratios=[4, 4, 4, 4], decoder_hidden_size=768, num_labels=150)
    torch.manual_seed(31)
    on = Vivim(in_chans=3, out_chans=3, depths=[1, 1, 1, 1], backbone=SegformerForSemanticSegmentation(cfg), fused_decode_head=True)
    _randomise_head(on.decoder, 32)
    off = copy.deepcopy(on)
    off.fused_decode_head = False
    g = torch.Generator().manual_seed(33)
    states = tuple(torch.randn(2, c, h, h, generator=g) for c, h in zip(DIMS, (8, 4, 2, 1)))
    return on, off, states


def test_cpu_tensors_take_the_stock_path_bit_for_bit():
    on, off, states = _models()
    assert on.fused_decode_head is True and off.fused_decode_head is False
    on.eval(), off.eval()
    with torch.no_grad():
        torch.manual_seed(5)
        a = on.decode(states, 1, 2)
        rng_after = torch.get_rng_state()
        torch.manual_seed(5)
        b = off.decode(states, 1, 2)
    assert torch.equal(a, b) and torch.equal(rng_after, torch.get_rng_state())      # the coin flips were drawn
    on.train(), off.train()
    try:
        torch.manual_seed(6)
        a = on.decode(states, 1, 2)
        torch.manual_seed(6)
        b = off.decode(states, 1, 2)
        assert a.requires_grad and torch.equal(a, b)
    finally:
        on.eval(), off.eval()


def test_the_gate():
    """applies() is False in train mode, with grad enabled, and for CPU tensors; nothing else is consulted first."""
    from vivim_amd import decode_head
    on, _, states = _models()
    on.eval()
    assert decode_head.applies(on, states) is False              # grad enabled
    with torch.no_grad():
        assert decode_head.applies(on, states) is False          # CPU tensors
        on.train()
        try:
            assert decode_head.applies(on, states) is False
        finally:
            on.eval()


def test_fold_cache_rebuilds_after_a_change():
    from vivim_amd import decode_head
    on, _, _ = _models()
    model = copy.deepcopy(on).eval()
    first = decode_head._folded(model)
    assert decode_head._folded(model) is first                  # nothing changed: the cached fold
    with torch.no_grad():
        model.decoder.batch_norm.running_mean.add_(1.0)
    second = decode_head._folded(model)
    assert second is not first and not torch.equal(second["bias"], first["bias"])
    assert torch.equal(second["bias"], decode_head.fold_decode_head(model.decoder, model.out)[1])
    state = {k: v.clone() for k, v in model.state_dict().items()}
    state["decoder.linear_fuse.weight"] = state["decoder.linear_fuse.weight"] * 2.0
    model.load_state_dict(state)
    third = decode_head._folded(model)
    assert third is not second and torch.equal(third["weights"][torch.float32][0], second["weights"][torch.float32][0] * 2.0)
    assert decode_head._folded(model) is third
    with torch.no_grad():
        model.out.bias.zero_()
    assert decode_head._folded(model) is not third and not decode_head._folded(model)["b_out"].any()
