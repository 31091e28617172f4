"""CPU: the validation-metrics entry points (include/vivim_hip.h: vivim_seg_metrics_params) are declared, exported and present,
the ctypes mirror has the library's layout, every bad argument is refused on the host before any launch, and the eager path of
vivim_amd/seg_metrics.py reproduces the fixtures written by the reference's own tracker (tests/golden/make_golden_seg_metrics.py).

Tolerances.  Counts are integers: compared exactly.  Metric values are fp64 quotients of integers (at most two roundings each)
and per-class sums of at most seven of them in [0, 1], divided once: absolute 1e-12 is four orders above that roundoff and
eight below the smallest change one pixel can make in these fixtures (1 / 65^2)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from vivim_amd import _lib

NAMES = ("vivim_seg_metrics", "vivim_seg_metrics_workspace_bytes")
OK, INVALID, UNSUPPORTED = 0, 1, 2
PTR = 1 << 20                                    # a non-null, 16-byte aligned address: no check may dereference it
FN = "vivim_seg_metrics"
FIXTURES = ("segm_c3_ties", "segm_c2_1x1", "segm_c8_odd", "segm_c3_unpredicted")
METRICS = ("dice", "jaccard", "precision", "recall", "f_measure", "specificity")
ATOL = 1e-12


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def check_results(res, fx, what=""):
    """A tracker's get_results() against the reference's recorded one: None exactly where it has None, values to ATOL."""
    C = fx["per_class"].shape[1]
    assert res["class_counts"] == [int(v) for v in fx["class_counts"]], what
    assert all(type(v) is int for v in res["class_counts"])
    for j, m in enumerate(METRICS):
        got = res[m]["per_class"]
        assert len(got) == C
        for c in range(C):
            want = fx["per_class"][j, c]
            if np.isnan(want):
                assert got[c] is None, (what, m, c)
            else:
                assert type(got[c]) is float and abs(got[c] - want) <= ATOL, (what, m, c, got[c], want)
        assert abs(res[m]["mean"] - fx["mean"][j]) <= ATOL, (what, m, res[m]["mean"], fx["mean"][j])


def test_symbols_declared_exported_and_present():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vivim_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vivim_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTS and hasattr(L, n), n
    assert "vivim_seg_metrics_params" in text


def test_struct_layout_and_abi_version():
    L = _lib.lib()
    assert L.vivim_sizeof(13) == ctypes.sizeof(_lib.SegMetricsParams) > 0
    assert L.vivim_sizeof(99) == 0
    assert L.vivim_abi_version() == 8


def _sizes(N=2, C=3, HW=35, itype=_lib.F32, ttype=0):
    P = _lib.SegMetricsParams()
    P.batch, P.classes, P.pixels, P.itype, P.ttype = N, C, HW, itype, ttype
    P.logits_batch_stride, P.logits_c_stride, P.target_batch_stride, P.pred_batch_stride = C * HW, HW, HW, HW
    return P


def _params(**kw):
    P = _sizes(**kw)
    P.logits = P.target = P.counts = P.pred = P.state = P.workspace = PTR
    P.workspace_bytes = _lib.lib().vivim_seg_metrics_workspace_bytes(ctypes.byref(P))
    return P


def _refused(P, code, message=None):
    """`code` and nothing launched: the pointers are not memory, so a kernel that started would not return an error code."""
    L = _lib.lib()
    assert L.vivim_seg_metrics(ctypes.byref(P), None) == code, L.vivim_last_error()
    assert L.vivim_last_error() != b""
    if message is not None:
        assert message in L.vivim_last_error(), L.vivim_last_error()


def test_null_struct_and_null_pointers():
    L = _lib.lib()
    assert L.vivim_seg_metrics(None, None) == INVALID and b"check failed" in L.vivim_last_error()
    assert L.vivim_seg_metrics_workspace_bytes(None) == 0
    for field in ("logits", "target", "counts"):
        P = _params()
        setattr(P, field, None)
        _refused(P, INVALID, b"check failed")
    P = _params()
    P.workspace = None
    _refused(P, INVALID, b"workspace")


def test_misaligned_pointers():
    for field, off in (("logits", 2), ("target", 4), ("counts", 2), ("state", 4), ("workspace", 2)):
        P = _params()                                                # f32 logits, int64 target
        setattr(P, field, PTR + off)
        _refused(P, INVALID)
    for itype in (_lib.BF16, _lib.F16):
        P = _params(itype=itype)
        P.logits = PTR + 1
        _refused(P, INVALID)


def test_bad_sizes_and_types():
    for field, v in (("pixels", 0), ("pixels", -3), ("batch", 0), ("batch", -1), ("itype", 3), ("itype", -1), ("ttype", 2),
                     ("ttype", -1)):
        P = _params()                                                # pointers and workspace of a good shape, then the bad value
        setattr(P, field, v)
        _refused(P, INVALID, b"check failed")


def test_workspace_one_byte_short():
    P = _params()
    P.workspace_bytes -= 1
    _refused(P, INVALID, b"vivim_seg_metrics_workspace_bytes")
    P.workspace_bytes = 0
    _refused(P, INVALID, b"workspace")


def test_unsupported_classes_carry_a_message():
    for C in (1, 9, 64):
        _refused(_params(C=C), UNSUPPORTED, b"2 to 8 classes")


def test_workspace_query_depends_on_sizes_only():
    L = _lib.lib()
    q = L.vivim_seg_metrics_workspace_bytes
    for kw in (dict(), dict(N=3, C=8, HW=5000, itype=_lib.BF16, ttype=1), dict(N=40, C=3, HW=512 * 512, itype=_lib.F16)):
        a, b = q(ctypes.byref(_sizes(**kw))), q(ctypes.byref(_params(**kw)))
        assert a == b > 0 and a % (4 * kw.get("N", 2) * 3 * kw.get("C", 3)) == 0
    # more pixels never need fewer slots, and the slot count per image is capped (the finalise kernel stays tiny)
    sizes = [q(ctypes.byref(_sizes(N=1, C=3, HW=hw))) for hw in (1, 1024, 1025, 4096, 1 << 20, 1 << 28)]
    assert sizes == sorted(sizes) and sizes[0] == 4 * 9 and sizes[1] < sizes[2] and sizes[-1] == sizes[-2]
    for bad in (dict(N=0), dict(HW=0), dict(C=0), dict(itype=5)):
        assert q(ctypes.byref(_sizes(**bad))) == 0


def test_algorithmic_bytes_has_a_branch_for_the_new_name():
    P = _sizes(N=2, C=3, HW=100, itype=_lib.BF16, ttype=1)
    assert _lib.algorithmic_bytes(FN, P) == 200 * (3 * 2 + 1) + 12 * 6
    P.pred = PTR
    assert _lib.algorithmic_bytes(FN, P) == 200 * (3 * 2 + 1 + 1) + 12 * 6
    P = _sizes(N=2, C=3, HW=100, itype=_lib.F32, ttype=0)
    assert _lib.algorithmic_bytes(FN, P) == 200 * (3 * 4 + 8) + 12 * 6


def test_exported_from_the_package():
    import vivim_amd
    from vivim_amd import seg_metrics
    assert vivim_amd.SegMetricsTracker is seg_metrics.SegMetricsTracker
    assert vivim_amd.seg_confusion_counts is seg_metrics.seg_confusion_counts
    with pytest.raises(AttributeError):
        vivim_amd.no_such_name


def test_supported_is_false_for_cpu_tensors():
    from vivim_amd import seg_metrics
    fx = load_fixture("segm_c3_ties")
    logits, targets = torch.from_numpy(fx["logits"]), torch.from_numpy(fx["targets"])
    assert seg_metrics.supported(logits, targets, 3) is False
    assert seg_metrics.supported(logits, targets.to(torch.uint8), 3) is False


@pytest.mark.parametrize("dt", ("fp32", "bf16"))
@pytest.mark.parametrize("name", FIXTURES)
def test_cpu_tensors_reproduce_the_reference_tracker(name, dt):
    from vivim_amd import seg_metrics
    fx = load_fixture(name)
    dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[dt]
    logits, targets = torch.from_numpy(fx["logits"]).to(dtype), torch.from_numpy(fx["targets"])
    assert torch.equal(logits.float(), torch.from_numpy(fx["logits"]))               # the fixtures are exact in every logit type
    C = logits.shape[1]
    counts, pred = seg_metrics.seg_confusion_counts(logits, targets, C, return_preds=True)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == tuple(fx["counts"].shape)
    assert np.array_equal(counts.numpy().astype(np.int64), fx["counts"])
    assert pred.dtype == torch.uint8 and np.array_equal(pred.numpy(), fx["logits"].argmax(axis=1))
    assert torch.equal(seg_metrics.seg_confusion_counts(logits, targets, C), counts)
    tracker = seg_metrics.SegMetricsTracker(num_classes=C)
    for a, b in fx["calls"]:
        tracker.update(logits[a:b], targets[a:b])
    assert tracker.state.dtype == torch.float64 and tuple(tracker.state.shape) == (C, 7)
    check_results(tracker.get_results(), fx, name)
    tracker.reset()
    assert not bool(tracker.state.any()) and tracker.get_results()["class_counts"] == [0] * C
    assert tracker.get_results()["dice"] == {"per_class": [None] * C, "mean": 0.0}


def test_clip_shaped_batches_are_taken_by_view():
    from vivim_amd import seg_metrics
    fx = load_fixture("segm_c3_unpredicted")                                          # N = 4: (B, T) = (2, 2)
    logits, targets = torch.from_numpy(fx["logits"]), torch.from_numpy(fx["targets"])
    tracker = seg_metrics.SegMetricsTracker(num_classes=3)
    tracker.update(logits.view(2, 2, *logits.shape[1:]), targets.view(2, 2, *targets.shape[1:]))
    check_results(tracker.get_results(), fx)


def test_eval_step_exists_and_the_tracker_is_optional():
    from vivim_amd import train_step
    sig = inspect.signature(train_step.eval_step).parameters
    assert list(sig)[:4] == ["model", "clip", "onehot", "num_classes"]
    assert sig["tracker"].default is None and sig["fused_loss"].default is False and sig["amp_dtype"].default is torch.bfloat16
    assert inspect.signature(train_step.train_step).parameters["fused_loss"].default is False
