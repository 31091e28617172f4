"""CPU: the binary recipe's validation metrics below the GPU.  include/vivim_hip_ext_binary_metrics.h parses into its row of
_lib.EXTENSIONS (what the registry as a whole holds: test_abi_extensions.py); the struct's layout is the C compiler's; the library
exports the two symbols; every host-side refusal carries its message; the eager composition and binary_metrics_cases.restate64 reproduce the
fixtures written by the reference's own classes; the tracker and eval_step_binary on the CPU."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import binary_metrics_cases as bc
from abi_cases import PTR, layout_matches_c, refused
from conftest import ROOT
from vivim_amd import _lib
from vivim_amd import binary_metrics as bm

HEADER = os.path.join(ROOT, "include", "vivim_hip_ext_binary_metrics.h")
NAMES = ("vivim_binary_metrics_workspace_bytes", "vivim_binary_metrics")
P = _lib.BinaryMetricsParams
FIELDS = ["struct_bytes", "batch", "height", "width", "ptype", "gtype", "pred_batch_stride", "gt_batch_stride", "pred", "gt",
          "thresholds", "values", "hist", "state", "workspace", "workspace_bytes"]
FIXTURES = bc.fixtures()
SWEEP_AND_E = [0, 1, 2, 3, 4, 5, 7]


# ---- the header and the tables

def test_the_header_parses_into_one_struct_and_two_entries():
    text = open(HEADER).read()
    assert "#ifndef VIVIM_HIP_EXT_BINARY_METRICS_H" in text and '#include "vivim_hip.h"' in text
    consts, classes, parsed = _lib.parse_header(text, {"vivim_binary_metrics_params": "BinaryMetricsParams"})
    assert consts == {} and list(classes) == ["BinaryMetricsParams"] and tuple(parsed) == NAMES
    ptr = ctypes.POINTER(classes["BinaryMetricsParams"])
    assert parsed[NAMES[0]] == _lib.Entry(None, (ptr,), False, ctypes.c_size_t)
    assert parsed[NAMES[1]] == _lib.Entry(None, (ptr,), True, ctypes.c_int)
    names, entries = _lib.EXTENSIONS["vivim_hip_ext_binary_metrics.h"]
    assert names == {"vivim_binary_metrics_params": "BinaryMetricsParams"} and tuple(entries) == NAMES
    assert entries == {NAMES[0]: _lib.Entry(None, (ctypes.POINTER(P),), False, ctypes.c_size_t),
                       NAMES[1]: _lib.Entry(None, (ctypes.POINTER(P),), True, ctypes.c_int)}
    assert [n for n, _ in P._fields_] == FIELDS and ctypes.sizeof(P) == 104
    types = dict(P._fields_)
    assert types["pred_batch_stride"] is ctypes.c_int64 and types["thresholds"] is ctypes.c_void_p and types["gtype"] is ctypes.c_int32


def test_the_library_exports_the_two_symbols():
    L = _lib.lib()
    assert getattr(L, NAMES[0]).argtypes == [ctypes.POINTER(P)] and getattr(L, NAMES[0]).restype is ctypes.c_size_t
    assert getattr(L, NAMES[1]).argtypes == [ctypes.POINTER(P), ctypes.c_void_p] and getattr(L, NAMES[1]).restype is ctypes.c_int


def test_layout_matches_the_c_compiler(tmp_path):
    layout_matches_c("vivim_hip_ext_binary_metrics.h", "vivim_binary_metrics_params", P, tmp_path)


# ---- refusals

def _good(**over):
    """Two fp32 maps of (5, 7) with float masks, every pointer present and aligned, a workspace of the size the query states."""
    p = P()
    p.struct_bytes = ctypes.sizeof(P)
    p.batch, p.height, p.width, p.ptype, p.gtype = 2, 5, 7, _lib.F32, _lib.F32
    p.pred_batch_stride = p.gt_batch_stride = 35
    p.pred = p.gt = p.thresholds = p.values = p.hist = p.state = p.workspace = PTR
    p.workspace_bytes = 1 << 20
    for k, v in over.items():
        setattr(p, k, v)
    return p


# the refusal of vivim_binary_metrics for `p` (the workspace query answers 0 for what it refuses itself)
_refused = functools.partial(refused, "vivim_binary_metrics")


def test_refusals_before_any_launch():
    L = _lib.lib()
    assert "binary_metrics: params is NULL" in _refused(None)
    assert "struct_bytes = 0, this library's vivim_binary_metrics_params has 104" in _refused(_good(struct_bytes=0))
    assert "struct_bytes = 112" in _refused(_good(struct_bytes=112))
    assert "ptype = 3: pred is fp32 / fp16 / bf16" in _refused(_good(ptype=3))
    for v in (4, -1):
        assert f"gtype = {v}: gt is fp32 / fp16 / bf16 (0 / 1 / 2) or uint8 / bool (3)" in _refused(_good(gtype=v))
    for field in ("batch", "height", "width"):
        for v in (0, -3):
            assert f"{field} = {v}" in _refused(_good(**{field: v})), field
    assert "height * width = 1: the metrics need at least 2 pixels" in _refused(_good(height=1, width=1))
    big = dict(pred_batch_stride=1 << 40, gt_batch_stride=1 << 40)
    assert "the index range overflows int32" in _refused(_good(height=1 << 16, width=1 << 15, **big))
    assert "the index range overflows int32" in _refused(_good(batch=1 << 27, **big))
    assert "pred_batch_stride = 34, gt_batch_stride = 35: an image has 35 elements" in _refused(_good(pred_batch_stride=34))
    assert "gt_batch_stride = 0" in _refused(_good(gt_batch_stride=0))
    for q in (None, _good(struct_bytes=0), _good(ptype=3), _good(height=1, width=1), _good(batch=1 << 27, **big)):
        assert L.vivim_binary_metrics_workspace_bytes(ctypes.byref(q) if q is not None else None) == 0
    assert L.vivim_binary_metrics_workspace_bytes(ctypes.byref(_good())) > 0
    for field in ("pred", "gt", "thresholds", "values"):
        assert f"{field} at (nil)" in _refused(_good(**{field: None})), field
    assert "pred at 0x1002: need a 4-byte aligned pointer" in _refused(_good(pred=PTR + 2))
    assert "pred at 0x1001: need a 2-byte aligned pointer" in _refused(_good(pred=PTR + 1, ptype=_lib.BF16))
    assert "gt at 0x1001: need a 2-byte aligned pointer" in _refused(_good(gt=PTR + 1, gtype=_lib.F16))
    assert "thresholds at 0x1002" in _refused(_good(thresholds=PTR + 2))
    assert "values at 0x1004: need an 8-byte aligned pointer" in _refused(_good(values=PTR + 4))
    assert "hist at 0x1002: need NULL or a 4-byte aligned pointer" in _refused(_good(hist=PTR + 2))
    assert "state at 0x1004: need NULL or an 8-byte aligned pointer" in _refused(_good(state=PTR + 4))
    need = L.vivim_binary_metrics_workspace_bytes(ctypes.byref(_good()))
    for over in (dict(workspace=None), dict(workspace=PTR + 4), dict(workspace_bytes=need - 1), dict(workspace_bytes=-1)):
        text = _refused(_good(**over))
        assert f"need a 8-byte aligned one of vivim_binary_metrics_workspace_bytes() = {need}" in text, over


def test_a_byte_mask_at_an_odd_address_is_not_refused_for_its_alignment():
    assert "values at (nil)" in _refused(_good(gt=PTR + 1, gtype=3, values=None))


# ---- the definition against the reference's fixtures

def test_the_fixtures_cover_the_cases():
    shapes = {tuple(f["pred"].shape[1:]) for f in FIXTURES.values()}
    assert shapes == {(1, 2), (5, 7), (33, 70), (64, 64), (97, 131)} and len(FIXTURES) == 11
    for name, f in FIXTURES.items():
        n = f["pred"].shape[0]
        assert f["pred"].dtype == np.float32 and f["gt"].dtype == np.uint8 and f["values"].shape == (n, 9), name
        assert f["counts"].shape == (n, 256, 4) and f["e_fg"].shape == f["e_bg"].shape == (n, 256), name
        assert os.path.getsize(os.path.join(bc.GOLDEN, f"binm_{name}.npz")) < 32 * 1024, name
    e = FIXTURES["edges_33x70"]
    G = e["gt"].reshape(6, -1).sum(1).tolist()
    assert G[0] == 0 and G[1] == 33 * 70 and G[4] == 1 and G[5] == 33 * 70 - 1 and e["pred"][2].min() == e["pred"][2].max()
    assert e["gt"][3][:, :-1].sum() == 0 and e["gt"][3][:, -1].sum() > 1 and e["values"][3:, 6].tolist() == [0.0, 0.0, 0.0]
    assert np.isin(FIXTURES["thresholds_33x70"]["pred"], bc.THRESHOLDS).all()


def _check_against_fixture(name, f, values, hists, what):
    """Integers exactly; sweep and E-measure to 1e-12; MAE and S-measure, which the reference computes in fp32, within 4 x the
    largest distance measured between it and restate64 over these fixtures (binary_metrics_cases.REFERENCE_FP32_GAP)."""
    for n in range(f["pred"].shape[0]):
        counts, e_fg, e_bg = hists[n]
        assert np.array_equal(counts, f["counts"][n]), (what, name, n)
        assert np.array_equal(e_fg, f["e_fg"][n]) and np.array_equal(e_bg, f["e_bg"][n]), (what, name, n)
        err = np.abs(values[n] - f["values"][n])
        assert err[SWEEP_AND_E].max() <= 1e-12, (what, name, n, err)
        assert err[6] <= 4 * bc.REFERENCE_FP32_GAP["Smeasure"] and err[8] <= 4 * bc.REFERENCE_FP32_GAP["MAE"], (what, name, n, err)
    return np.abs(values - f["values"]).max(0)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_restate64_reproduces_the_reference(name):
    f = FIXTURES[name]
    res = [bc.restate64(f["pred"][n], f["gt"][n] != 0) for n in range(f["pred"].shape[0])]
    worst = _check_against_fixture(name, f, np.stack([r["values"] for r in res]), [(r["counts"], r["e_fg"], r["e_bg"]) for r in res], "restate64")
    print(f"restate64[{name}]: worst |restate64 - reference|: Smeasure {worst[6]:.3e}, MAE {worst[8]:.3e}, the rest {worst[SWEEP_AND_E].max():.3e}")
    for n, r in enumerate(res):                  # the sweep's histogram and its per-threshold counts say the same
        S, G = f["gt"][n].size, int((f["gt"][n] != 0).sum())
        assert np.array_equal(bc.counts_from_hist(np.stack([r["sweep_fg"], r["sweep_bg"], r["e_fg"], r["e_bg"]]), G, S)[0], r["counts"])


def test_the_recorded_gap_is_the_measured_one():
    """REFERENCE_FP32_GAP is the largest |reference - restate64| over the fixtures, rounded up by less than 2 %."""
    gap = {"Smeasure": 0.0, "MAE": 0.0}
    for f in FIXTURES.values():
        for n in range(f["pred"].shape[0]):
            v = bc.restate64(f["pred"][n], f["gt"][n] != 0)["values"]
            gap["Smeasure"] = max(gap["Smeasure"], abs(v[6] - f["values"][n][6]))
            gap["MAE"] = max(gap["MAE"], abs(v[8] - f["values"][n][8]))
    for k, v in gap.items():
        assert v <= bc.REFERENCE_FP32_GAP[k] <= 1.02 * v, (k, v)


@pytest.mark.parametrize("gt_dtype", [torch.uint8, torch.bool, torch.float32])
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_the_eager_composition_reproduces_the_reference(name, gt_dtype):
    f = FIXTURES[name]
    pred, gt = torch.from_numpy(f["pred"]), torch.from_numpy(f["gt"]).to(gt_dtype)
    assert not bm.supported(pred, gt)
    values, hist = bm.binary_image_metrics(pred, gt, return_hist=True)
    assert values.dtype == torch.float64 and hist.dtype == torch.int32 and hist.shape == (pred.shape[0], 4, 256)
    hists = [bc.counts_from_hist(hist[n].numpy(), int((f["gt"][n] != 0).sum()), f["gt"][n].size) for n in range(pred.shape[0])]
    _check_against_fixture(name, f, values.numpy(), hists, "eager")
    for n in range(pred.shape[0]):               # and restate64, the same definition: same integers, rounding apart
        r = bc.restate64(f["pred"][n], f["gt"][n] != 0)
        x = bc.restate_exact(f["pred"][n], f["gt"][n] != 0)
        assert np.array_equal(hist[n, 0].numpy(), r["sweep_fg"]) and np.array_equal(hist[n, 1].numpy(), r["sweep_bg"])
        err = np.abs(values[n].numpy() - r["values"])
        assert err[SWEEP_AND_E].max() <= 1e-12 and err[8] <= f["gt"][n].size * 2.0 ** -53
        assert err[6] <= 1e-12 + 64 * abs(r["values"][6] - x["values"][6])


def test_sixteen_bit_maps_and_other_shapes_say_the_same():
    f = FIXTURES["prob_33x70"]
    assert int(f["all_dtypes"]) == 1
    pred, gt = torch.from_numpy(f["pred"]), torch.from_numpy(f["gt"])
    want = bm.binary_image_metrics(pred, gt)
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(bm.binary_image_metrics(pred.to(dt), gt.to(dt)), want)
    assert torch.equal(bm.binary_image_metrics(pred[:, None], gt[:, None]), want)
    assert torch.equal(bm.binary_image_metrics(pred[None, :, None], gt[None, :, None]), want)
    assert torch.equal(bm.binary_image_metrics(pred.transpose(1, 2).contiguous().transpose(1, 2), gt), want)
    assert bm.binary_image_metrics(pred[:0], gt[:0]).shape == (0, 9)
    with pytest.raises(AssertionError):
        bm.binary_image_metrics(pred, gt[:1])
    with pytest.raises(AssertionError):
        bm.binary_image_metrics(pred[:, :1, :1], gt[:, :1, :1])


def test_the_constant_quadrant_takes_the_one_branch():
    pred, gt = bc.constant_quadrant()
    r, x = bc.restate64(pred[0], gt[0]), bc.restate_exact(pred[0], gt[0])
    got = bm.binary_image_metrics(torch.from_numpy(pred), torch.from_numpy(gt))[0, 6].item()
    assert abs(got - r["values"][6]) <= 1e-12 + 64 * abs(r["values"][6] - x["values"][6])
    # with a rounding error in that quadrant's variance the quadrant would score 0: half its weight less
    wrong = r["values"][6] - 0.5 * (33 * 17) / (33 * 70)
    assert abs(got - wrong) > 0.1


# ---- the tracker and the step

def test_the_tracker_on_the_cpu():
    f, e = FIXTURES["prob_5x7"], FIXTURES["bin_5x7"]
    tracker = bm.BinaryMetricsTracker()
    assert tracker.state.shape == (10,) and tracker.state.dtype == torch.float64 and tracker.get_results() == dict.fromkeys(bm.VALUES, 0.0)
    tracker.update(torch.from_numpy(f["pred"]), torch.from_numpy(f["gt"]))
    tracker.update(torch.from_numpy(e["pred"])[:0], torch.from_numpy(e["gt"])[:0])                       # an empty batch: nothing
    tracker.update(torch.from_numpy(e["pred"]).view(1, 3, 1, 5, 7), torch.from_numpy(e["gt"]).view(1, 3, 1, 5, 7))
    one = bm.BinaryMetricsTracker()
    one.update(torch.from_numpy(np.concatenate([f["pred"], e["pred"]])), torch.from_numpy(np.concatenate([f["gt"], e["gt"]])))
    assert torch.equal(one.state, tracker.state) and tracker.state[9].item() == 6.0
    res = tracker.get_results()
    assert list(res) == ["Dice", "Jaccard", "Precision", "Recall", "Fmeasure", "specificity", "Smeasure", "Emeasure", "MAE"]
    want = np.concatenate([f["values"], e["values"]]).mean(0)
    for k, name in enumerate(bm.VALUES):
        assert abs(res[name] - want[k]) <= (4 * max(bc.REFERENCE_FP32_GAP.values()) if k in (6, 8) else 1e-12), name
    tracker.reset()
    assert not tracker.state.any()
    import vivim_amd
    assert vivim_amd.BinaryMetricsTracker is bm.BinaryMetricsTracker and vivim_amd.binary_image_metrics is bm.binary_image_metrics


class _StandIn(torch.nn.Module):
    """(B, nf, 3, H, W) -> (B * nf, 1, H, W) logits, as the binary model's forward."""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 1, 3, padding=1)

    def forward(self, clip):
        return self.conv(clip.flatten(0, 1))


@pytest.mark.parametrize("frames", ["center", "all"])
def test_eval_step_binary_on_a_stand_in_model(frames):
    from vivim_amd import structure_loss as sl
    from vivim_amd import train_step
    torch.manual_seed(5)
    model = _StandIn()
    clip = torch.randn(2, 3, 3, 8, 9)
    mask = torch.from_numpy(bc.blob_mask(np.random.default_rng(6), 6, 8, 9)).float().view(2, 3, 1, 8, 9)
    tracker = bm.BinaryMetricsTracker()
    loss = train_step.eval_step_binary(model, clip, mask, tracker=tracker, amp_dtype=torch.float32, frames=frames)
    assert not model.training and not loss.requires_grad and loss.dim() == 0
    with torch.no_grad():
        logits, target = model(clip), mask.view(6, 1, 8, 9)
    if frames == "center":
        logits, target = logits[1::3], target[1::3]
    assert torch.equal(loss, sl.structure_loss(logits, target))
    want = bm.BinaryMetricsTracker()
    want.update((torch.sigmoid(logits) > 0.5).float(), target)
    assert torch.equal(tracker.state, want.state) and tracker.state[9].item() == (2.0 if frames == "center" else 6.0)
    assert torch.equal(train_step.eval_step_binary(model, clip, mask, amp_dtype=torch.float32, frames=frames), loss)      # no tracker
    with pytest.raises(AssertionError):
        train_step.eval_step_binary(model, clip, mask, amp_dtype=torch.float32, frames="first")
