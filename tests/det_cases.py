"""Case tables of tests/test_gpu_deterministic_edges.py: the shapes at which a slot of the deterministic backward kernels (csrc/det.cuh)
could stay unwritten, be written twice or land on the wrong element -- batch 1, several B/C groups, odd channel counts, ragged channel
blocks, rows below one tile and of whole tiles plus a little, strided and sliced rows, optional inputs off.

Geometry the shapes are chosen against (read from the kernels; a workgroup's share of a B/C group):
    generic (scan_bwd.hip, ssm_bwd_generic_kernel)    one wave per channel pair, 4 waves per workgroup, 256-token steps
    lanes = tokens (ssm_bwd_fast_kernel)              one wave per channel pair, 4 or 8 waves per workgroup, steps of 64 * K tokens
                                                      with K = 8 unless the last 512-token step would be mostly empty (then 4);
                                                      the deterministic call runs K = 8 with 4-wave workgroups whatever is pinned
    lanes = states (scan_ls.hip, scan_ls2.hip)        16 * (64 / dstate) channels per wave, up to 4 waves per workgroup: 64 channels
                                                      at dstate 16, 16 at dstate 64; 16-token tiles; dB / dC go through slots only when
                                                      a group has more than two workgroups (two adds commute)
"""
import collections

import torch

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16

# states_bpg: workgroups per B/C group of the lanes = states kernels at this shape, ceil(dim / groups / channels per workgroup).
ScanCase = collections.namedtuple("ScanCase", "batch dim groups dstate seqlen dtype strided opts init states_bpg")


def _scan(batch, dim, groups, dstate, seqlen, dtype, states_bpg=None, strided=False, init="module", **opts):
    return ScanCase(batch, dim, groups, dstate, seqlen, dtype, strided, opts, init, states_bpg)


SCAN_CASES = {
    # batch 1, three groups, a row shorter than any tile: every workgroup is the only contributor of its group
    "b1_g3_short": _scan(1, 192, 3, 16, 8, BF16, states_bpg=1),
    # channel blocks 64 + 32, five 256-token rows + 8: two lanes = states workgroups per group, the unslotted pair of adds
    "ragged_pair": _scan(2, 96, 1, 16, 1288, F32, states_bpg=2),
    # 3 x 64 + 16 channels: four lanes = states workgroups per group, slotted dB / dC with a ragged last block
    "slotted_ragged": _scan(2, 208, 1, 16, 1288, BF16, states_bpg=4),
    # the same rows with whole blocks and two workgroups per group: the size test_det_scan_states_slots_add_to_the_size compares with
    "pair_whole": _scan(2, 128, 1, 16, 1288, BF16, states_bpg=2),
    # 200 = 3 x 64 + 8 channels per group, three groups: the slot index depends on the group offset
    "slotted_g3": _scan(1, 600, 3, 16, 520, F16, states_bpg=4),
    # 75 channels per group: a shadow channel, and 38 channel pairs over 4-wave workgroups (the last one with two surplus waves)
    "odd_cpg": _scan(2, 225, 3, 16, 264, F32, states_bpg=2),
    # ... over 8-wave workgroups.  At 264 tokens the lanes = tokens kernel takes 8 tokens per lane and the deterministic call then
    # runs 4-wave workgroups whatever is pinned; 520 tokens (two 256-token steps + 8) is the nearest row that keeps 4 tokens per
    # lane and with them the pinned 8 waves: 38 pairs = 4 x 8 + 6, two surplus waves in the last workgroup
    "odd_cpg_w8": _scan(2, 225, 3, 16, 520, F32, states_bpg=2),
    # dstate 64, ragged blocks: 16 channels per first-generation lanes = states workgroup, 16 + 16 + 8 slotted
    "n64_ragged": _scan(2, 40, 1, 64, 264, BF16, states_bpg=3),
    "n64_g2": _scan(1, 80, 2, 64, 72, F16, states_bpg=3),
    # many segments, a ragged block, batch 1: the (batch, segment) slot index.  Built as Vivim's (L, B*L, 1)-strided rows, which
    # with one batch element lie in memory like contiguous ones
    "long_strided": _scan(1, 80, 1, 16, 20480, BF16, states_bpg=2, strided=True),
    # optional inputs off in turn: the dD / dbias slot regions unused, the no-z instantiations.  Without softplus delta itself is the
    # step size, so the reference tests' distribution (all positive) stands in for the module's
    "no_z": _scan(3, 208, 1, 16, 1288, BF16, states_bpg=4, has_z=False),
    "no_D_no_bias": _scan(3, 208, 1, 16, 1288, BF16, states_bpg=4, has_D=False, has_bias=False),
    "no_softplus": _scan(3, 208, 1, 16, 1288, BF16, states_bpg=4, init="test", softplus=False),
    # what only the generic kernel takes: odd channel counts, dstate 1 / 3 / 24 / 200, one token
    "tiny_odd": _scan(2, 5, 1, 3, 3, F32),
    "one_token": _scan(1, 4, 1, 1, 1, F32),
    "n24_g2": _scan(2, 10, 2, 24, 151, BF16),
    "n200_g2": _scan(1, 8, 2, 200, 40, F32),
}

_EVERY = ["b1_g3_short", "ragged_pair", "slotted_ragged", "slotted_g3", "long_strided", "no_z", "no_D_no_bias", "no_softplus"]
# Per family (test_gpu_deterministic.FAMILIES), the cases it can take.  states2 (dstate 16 only) has no dstate-64 case; tokens_w8
# has odd_cpg_w8 in the place of odd_cpg (see there); the last four are refused by every family but the generic one (the
# lanes = states kernels take dstate 16 / 32 / 64, the lanes = tokens kernel dstate <= 64 and rows of whole 4-token lanes).
SCAN_FAMILY_CASES = {
    "tokens_w8": _EVERY + ["odd_cpg_w8", "n64_ragged", "n64_g2"],
    "tokens_w4": _EVERY + ["odd_cpg", "n64_ragged", "n64_g2"],
    "generic": _EVERY + ["odd_cpg", "n64_ragged", "n64_g2", "tiny_odd", "one_token", "n24_g2", "n200_g2"],
    "states1": _EVERY + ["odd_cpg", "n64_ragged", "n64_g2"],
    "states2": _EVERY + ["odd_cpg"],
}

# Constant B / C, (dim, dstate) tensors (generic family): (batch, dim, dstate, seqlen, dtype)
CONST_BC_CASES = [(1, 5, 16, 37, F32), (3, 130, 16, 300, BF16)]

# ---- causal conv1d.  The channel-first deterministic kernel covers 256 lanes x 16 bytes per tile: 1024 fp32 or 2048 16-bit tokens.
# (batch, dim, seqlen, width, layout); layout "plain": contiguous, "slice": a channel slice of a wider tensor (unaligned row starts for
# an odd row length), "xz": Vivim's (L, B*L, 1) layout, the first half of xz, with dx written into a caller-owned view.
CONV_CASES = [
    (1, 1, 1, 2, "plain"),
    (2, 7, 3, 4, "plain"),                    # a row shorter than the filter
    (3, 130, 2049, 4, "plain"),               # two tiles (fp32) or one (bf16) plus one token
    (2, 96, 151, 3, "slice"),
    (3, 64, 1280, 4, "xz"),
]
# channel-last (csrc/conv1d_cl.hip, slots per (batch, chunk)); "slice": a channel slice of a wider channel-last tensor, a token stride
# wider than the row
CONV_CL_CASES = [
    (2, 30, 151, 3, "plain"),
    (1, 257, 700, 2, "plain"),
    (3, 64, 2049, 4, "plain"),
    (2, 30, 151, 3, "slice"),
]
CONV_OPTIONS = [(True, True), (True, False), (False, True), (False, False)]        # (bias, SiLU)

# ---- depthwise-conv weight gradient: (B, C, D, H, W, bias).  A block takes 128 channels and 4 waves x 8 tiles of 4 positions
# along W; a slot per (batch, block along the tiles).
DWCONV_CASES = [
    (1, 40, 1, 7, 5, True),
    # two channel groups, the second with two channels, a width that is no multiple of 4.  130 channels are outside what the forward
    # and dx kernels take (whole 16-byte vectors of channels): this case calls the weight-gradient entry point alone
    (2, 130, 3, 5, 7, True),
    (3, 8, 3, 1, 1, True),
    (1, 128, 1, 9, 12, False),
    # 45 tiles: two blocks along the tiles, the second with 13 tiles -- one full wave, one partial, two idle
    (2, 8, 3, 5, 9, True),
]
