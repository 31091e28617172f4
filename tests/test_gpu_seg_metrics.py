"""GPU: the validation-metrics kernels (vivim_amd/seg_metrics.py, csrc/seg_metrics.hip) against the fixtures written by the
reference's own tracker (tests/golden/segm_*.npz) and, for shapes beyond them, against the definition evaluated with numpy on the
host: `logits.float().cpu().numpy().argmax(1)`, then `==` and `sum`, all in integers.

Tolerances.  Counts and prediction maps are integers: compared EXACTLY.  Metric values are fp64, at most two roundings per value
and a sum of at most seven values in [0, 1] (no tracker here sees more than seven images): absolute 1e-12."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import DT
from test_abi_seg_metrics import ATOL, FIXTURES, check_results, load_fixture
from vivim_amd import _lib

pytestmark = pytest.mark.gpu

TT = {"int64": torch.int64, "uint8": torch.uint8}
ITYPE = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}


def host_counts(logits, targets):
    """(counts (N, C, 3) int64, pred (N, H, W)) by the definition, on the host."""
    x = logits.float().cpu().numpy()
    t = targets.cpu().numpy().astype(np.int64)
    pred = x.argmax(1)
    N, C = x.shape[:2]
    counts = np.zeros((N, C, 3), dtype=np.int64)
    for n in range(N):
        for c in range(C):
            tp = int(((pred[n] == c) & (t[n] == c)).sum())
            counts[n, c] = (tp, int((pred[n] == c).sum()) - tp, int((t[n] == c).sum()) - tp)
    return counts, pred


def host_state(counts, HW, state=None):
    """The (C, 7) fp64 state after these images, in image order, by the definition in Python floats."""
    N, C = counts.shape[:2]
    st = np.zeros((C, 7), dtype=np.float64) if state is None else state
    for n in range(N):
        for c in range(C):
            tp, fp, fn = (int(v) for v in counts[n, c])
            if tp + fn == 0:
                continue
            tn = HW - tp - fp - fn
            prec = 0.0 if tp + fp == 0 else tp / (tp + fp)
            rec = tp / (tp + fn)
            st[c] += np.array([2.0 * tp / (2 * tp + fp + fn), tp / (tp + fp + fn), prec, rec,
                               2.0 * prec * rec / (prec + rec + 1e-5), 0.0 if tp + fn == HW else tn / (tn + fp), 1.0])
    return st


def make_case(cuda, shape, dtype, seed=0, ttype=torch.int64):
    """Logits randn rounded to bf16 (exact in every logit type, and coarse enough that ties occur); image 0 has its last class
    relabelled, so one class is absent there."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed * 1000 + N * 100 + C * 10 + H)
    logits = torch.randn(N, C, H, W, generator=g).to(torch.bfloat16).to(dtype).to(cuda)
    targets = torch.randint(0, C, (N, H, W), generator=g)
    targets[0][targets[0] == C - 1] = 0
    return logits, targets.to(ttype).to(cuda)


def check_all(logits, targets, C, what, expect=None):
    """Counts, prediction map and a fresh tracker's state of one batch (at most seven images) against the host definition."""
    from vivim_amd import seg_metrics
    assert seg_metrics.supported(logits, targets, C), what
    want, want_pred = expect if expect is not None else host_counts(logits, targets)
    N, _, H, W = logits.shape
    assert N <= 7
    counts, pred = seg_metrics.seg_confusion_counts(logits, targets, C, return_preds=True)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (N, C, 3)
    assert pred.dtype == torch.uint8 and tuple(pred.shape) == (N, H, W)
    assert np.array_equal(pred.cpu().numpy(), want_pred), f"{what}: prediction map"
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), want), f"{what}: counts {counts.cpu().tolist()} want {want.tolist()}"
    assert torch.equal(seg_metrics.seg_confusion_counts(logits, targets, C), counts), what
    tracker = seg_metrics.SegMetricsTracker(num_classes=C)
    tracker.update(logits, targets)
    assert tracker.state.device == logits.device and tracker.state.dtype == torch.float64
    err = np.abs(tracker.state.cpu().numpy() - host_state(want, H * W)).max()
    assert err <= ATOL, f"{what}: state off by {err:.3e}"
    return counts, pred, tracker.state


@pytest.mark.parametrize("tt", list(TT))
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures(cuda, name, dt, tt):
    from vivim_amd import seg_metrics
    fx = load_fixture(name)
    logits = torch.from_numpy(fx["logits"]).to(DT[dt]).to(cuda)
    targets = torch.from_numpy(fx["targets"]).to(TT[tt]).to(cuda)
    assert torch.equal(logits.float().cpu(), torch.from_numpy(fx["logits"]))         # exact in every logit type
    C = logits.shape[1]
    check_all(logits, targets, C, name, expect=(fx["counts"], fx["logits"].argmax(axis=1)))
    tracker = seg_metrics.SegMetricsTracker(num_classes=C)
    for a, b in fx["calls"]:
        tracker.update(logits[a:b], targets[a:b])
    check_results(tracker.get_results(), fx, name)


@pytest.mark.parametrize("dt", list(DT))
def test_tails_and_tiny_images(cuda, dt):
    """Not a multiple of the 4- / 8-element vector, fewer pixels than one wave, one pixel past a workgroup (256 threads)."""
    for H, W in ((1, 1), (1, 3), (5, 7), (3, 11), (1, 255), (1, 257)):
        for tt in TT.values():
            logits, targets = make_case(cuda, (2, 3, H, W), DT[dt], seed=1, ttype=tt)
            check_all(logits, targets, 3, f"{H}x{W} {dt} {tt}")


def _blocks_per_image(C, pixels, dtype):
    P = _lib.SegMetricsParams()
    P.batch, P.classes, P.pixels, P.itype = 1, C, pixels, ITYPE[dtype]
    b = _lib.lib().vivim_seg_metrics_workspace_bytes(ctypes.byref(P))
    assert b > 0 and b % (4 * 3 * C) == 0
    return b // (4 * 3 * C)


@pytest.mark.parametrize("dt", list(DT))
def test_grid_stride_loop(cuda, dt):
    """The smallest square just above (slot cap x threads x elements per thread) pixels, so that the first workgroups go round
    their loop twice.  The figures come from the library's own workspace query (kSmMaxBlocks = 64 slots per image, kSmThreads =
    256, 16 bytes of logits per thread: 4 fp32 or 8 16-bit elements): 257 x 257 for fp32, 363 x 363 for fp16 / bf16."""
    dtype = DT[dt]
    cap = _blocks_per_image(3, 1 << 28, dtype)
    per_block = 1
    while _blocks_per_image(3, per_block + 1, dtype) < 2:
        per_block *= 2
    side = math.isqrt(cap * per_block) + 1
    assert (cap, per_block, side) == ((64, 1024, 257) if dtype == torch.float32 else (64, 2048, 363))
    assert _blocks_per_image(3, side * side, dtype) == cap and cap * per_block < side * side < (cap + 1) * per_block
    logits, targets = make_case(cuda, (1, 3, side, side), dtype, seed=2)
    check_all(logits, targets, 3, f"grid-stride {side}x{side} {dt}")


@pytest.mark.parametrize("dt", list(DT))
def test_scalar_paths(cuda, dt):
    """Views that no 16-byte vector can reach give the same counts and map as their packed copies."""
    dtype = DT[dt]
    N, C, H, W = 3, 3, 5, 7                                                          # 35 pixels: rows of 140 / 70 bytes
    packed, targets = make_case(cuda, (N, C, H, W), dtype, seed=3)
    want = host_counts(packed, targets)
    c0, p0, s0 = check_all(packed, targets, C, "packed", expect=want)
    assert p0[1].data_ptr() % 2 == 1                                                 # the map's rows start at odd byte offsets
    # a channel slice of a wider tensor
    wide = torch.full((N, C + 2, H, W), float("nan"), dtype=dtype, device=cuda)
    view = wide[:, 1:1 + C]
    view.copy_(packed)
    assert view.stride() == ((C + 2) * H * W, H * W, W, 1) and (H * W * packed.element_size()) % 16 != 0
    c1, p1, s1 = check_all(view, targets, C, "channel slice", expect=want)
    assert torch.equal(c1, c0) and torch.equal(p1, p0) and torch.equal(s1, s0)
    # the same logits one element into their storage, with rows that would otherwise be whole vectors
    N, C, H, W = 2, 3, 8, 16
    packed, targets = make_case(cuda, (N, C, H, W), dtype, seed=4)
    want = host_counts(packed, targets)
    c0, p0, s0 = check_all(packed, targets, C, "packed 8x16", expect=want)
    flat = torch.full((N * C * H * W + 1,), float("nan"), dtype=dtype, device=cuda)
    off = flat[1:].view(N, C, H, W)
    off.copy_(packed)
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()
    c1, p1, s1 = check_all(off, targets, C, "odd storage offset", expect=want)
    assert torch.equal(c1, c0) and torch.equal(p1, p0) and torch.equal(s1, s0)
    # targets as a view at an odd element offset
    for tt in TT.values():
        tflat = torch.full((N * H * W + 1,), 1, dtype=tt, device=cuda)
        tview = tflat[1:].view(N, H, W)
        tview.copy_(targets)
        assert tview.data_ptr() % 16 != 0
        c1, p1, s1 = check_all(packed, tview, C, f"target offset {tt}", expect=want)
        assert torch.equal(c1, c0) and torch.equal(p1, p0) and torch.equal(s1, s0)


@pytest.mark.parametrize("C", range(2, 9))
def test_classes(cuda, C):
    for dtype in (torch.float32, torch.bfloat16):
        logits, targets = make_case(cuda, (2, C, 7, 9), dtype, seed=5)
        check_all(logits, targets, C, f"C={C} {dtype}")


@pytest.mark.parametrize("dt", list(DT))
def test_special_values_follow_numpy_argmax(cuda, dt):
    """A NaN is the maximum and the first NaN wins; among equal maxima (+inf twice, -0.0 against 0.0, all equal) the first index."""
    nan, inf = float("nan"), float("inf")
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 3, 4, 8, generator=g).to(torch.bfloat16).float()
    x[0, 1, 0, :] = nan                                                              # NaN in class 1
    x[0, 0, 1, :] = nan                                                              # NaN in classes 0 and 2
    x[0, 2, 1, :] = nan
    x[0, 1, 2, :4] = nan                                                             # NaN in classes 1 and 2: class 1
    x[0, 2, 2, :4] = nan
    x[0, 2, 2, 4:] = nan                                                             # NaN in class 2 against a larger finite class
    x[0, 0, 2, 4:] = 100.0
    x[0, 1, 3, :] = inf                                                              # +inf in classes 1 and 2: class 1
    x[0, 2, 3, :] = inf
    x[1, :, 0, :] = 0.0                                                              # -0.0 (class 0) against 0.0: class 0
    x[1, 0, 0, :] = -0.0
    x[1, 0, 1, :] = 0.0                                                              # 0.0 (class 0) against -0.0
    x[1, 1:, 1, :] = -0.0
    x[1, :, 2, :] = 1.5                                                              # all equal
    x[1, :, 3, :4] = -inf                                                            # all -inf
    x[1, 0, 3, 4:] = -inf                                                            # -inf against NaN
    x[1, 1, 3, 4:] = nan
    want_pred = x.numpy().argmax(1)
    assert want_pred[0, 0].tolist() == [1] * 8 and want_pred[0, 1].tolist() == [0] * 8 and want_pred[0, 2].tolist() == [1] * 4 + [2] * 4
    assert want_pred[0, 3].tolist() == [1] * 8 and not want_pred[1, :3].any() and want_pred[1, 3].tolist() == [0] * 4 + [1] * 4
    logits = x.to(DT[dt]).to(cuda)
    targets = torch.randint(0, 3, (2, 4, 8), generator=g).to(cuda)
    check_all(logits, targets, 3, f"special values {dt}")
    _, pred, _ = check_all(logits, targets.to(torch.uint8), 3, f"special values {dt} uint8")
    assert np.array_equal(pred.cpu().numpy(), want_pred)


def test_labels_outside_the_classes_are_pixels_of_no_class(cuda):
    """They add to fp of the class predicted there and to nothing else: the same counts whatever the out-of-range value."""
    for dtype in (torch.float32, torch.float16):
        for shape in ((2, 3, 5, 7), (2, 3, 8, 16)):
            logits, t64 = make_case(cuda, shape, dtype, seed=7)
            g = torch.Generator().manual_seed(8)
            hole = (torch.rand(t64.shape, generator=g) < 0.25).to(cuda)
            base = None
            for tt, values in ((torch.int64, (3, 255, -1, 2 ** 40)), (torch.uint8, (3, 255))):
                for v in values:
                    targets = t64.masked_fill(hole, v).to(tt) if tt == torch.int64 else t64.to(tt).masked_fill(hole, v)
                    counts, _, _ = check_all(logits, targets, 3, f"label {v} {tt} {dtype} {shape}")
                    base = counts if base is None else base
                    assert torch.equal(counts, base), (v, tt)
            # against the labels without holes: tp and fn of the holes' classes went away, their predictions became fp
            full = host_counts(logits, t64)[0]
            b = base.cpu().numpy().astype(np.int64)
            assert (b[..., 0] + b[..., 1] == full[..., 0] + full[..., 1]).all() and (b[..., 0] <= full[..., 0]).all()
            assert (b[..., 2] <= full[..., 2]).all() and b[..., 2].sum() < full[..., 2].sum()


def test_accumulation_streams_and_reset(cuda):
    from vivim_amd import seg_metrics
    batches = [make_case(cuda, (2, 3, 9, 13), dt, seed=10 + i) for i, dt in enumerate((torch.float32, torch.float32, torch.float32))]
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    a, b = seg_metrics.SegMetricsTracker(3), seg_metrics.SegMetricsTracker(3)
    with torch.cuda.stream(side):
        for logits, targets in batches:
            a.update(logits, targets)
        res_a = a.get_results()
    side.synchronize()
    torch.cuda.current_stream(cuda).wait_stream(side)
    for logits, targets in batches:
        b.update(logits, targets)
    assert torch.equal(a.state, b.state)                                             # the same batches: the same bits
    one = seg_metrics.SegMetricsTracker(3)
    one.update(torch.cat([l for l, _ in batches]), torch.cat([t for _, t in batches]))
    res_one = one.get_results()
    want = np.zeros((3, 7))
    for logits, targets in batches:
        host_state(host_counts(logits, targets)[0], 9 * 13, want)
    assert np.abs(a.state.cpu().numpy() - want).max() <= ATOL and np.abs(one.state.cpu().numpy() - want).max() <= ATOL
    assert res_a["class_counts"] == res_one["class_counts"] == [int(v) for v in want[:, 6]]
    assert sum(res_a["class_counts"]) == 15                                        # 3 x (image 0: two classes, image 1: three)
    for m in ("dice", "jaccard", "precision", "recall", "f_measure", "specificity"):
        assert abs(res_a[m]["mean"] - res_one[m]["mean"]) <= ATOL
        for c in range(3):
            assert abs(res_a[m]["per_class"][c] - want[c, METRIC_COL[m]] / want[c, 6]) <= ATOL
    # clip-shaped batches are taken by view
    five = seg_metrics.SegMetricsTracker(3)
    l5, t5 = torch.cat([l for l, _ in batches[:2]]), torch.cat([t for _, t in batches[:2]])
    five.update(l5.view(2, 2, 3, 9, 13), t5.view(2, 2, 9, 13))
    two = seg_metrics.SegMetricsTracker(3)
    two.update(l5, t5)
    assert torch.equal(five.state, two.state)
    a.reset()
    assert not bool(a.state.any()) and a.get_results()["class_counts"] == [0, 0, 0]
    a.update(*batches[0])
    b.reset()
    b.update(*batches[0])
    assert torch.equal(a.state.cpu(), b.state.cpu()) and bool(a.state.any())


METRIC_COL = {"dice": 0, "jaccard": 1, "precision": 2, "recall": 3, "f_measure": 4, "specificity": 5}


def test_update_neither_synchronises_nor_copies_to_the_host(cuda):
    from vivim_amd import seg_metrics
    logits, targets = make_case(cuda, (2, 3, 16, 24), torch.bfloat16, seed=20)
    seg_metrics.seg_confusion_counts(logits, targets, 3)                             # the library is loaded, the device is up
    tracker = seg_metrics.SegMetricsTracker(3)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tracker.update(logits, targets)                                              # the first one also makes the state
        tracker.update(logits.view(1, 2, 3, 16, 24), targets.view(1, 2, 16, 24))
        counts, pred = seg_metrics.seg_confusion_counts(logits, targets, 3, return_preds=True)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    want = host_counts(logits, targets)
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), want[0]) and np.array_equal(pred.cpu().numpy(), want[1])
    st = host_state(want[0], 16 * 24, host_state(want[0], 16 * 24))
    assert np.abs(tracker.state.cpu().numpy() - st).max() <= ATOL
    assert tracker.get_results()["class_counts"] == [int(v) for v in st[:, 6]]


def test_fallbacks_take_the_eager_definition(cuda):
    from vivim_amd import seg_metrics
    l9, t9 = make_case(cuda, (2, 9, 7, 9), torch.float32, seed=21)
    logits, targets = make_case(cuda, (2, 3, 8, 8), torch.float32, seed=22)
    cl = logits.contiguous(memory_format=torch.channels_last)
    assert cl.stride(3) != 1
    for x, t, C in ((l9, t9, 9), (cl, targets, 3), (logits.double(), targets, 3), (logits, targets.int(), 3)):
        assert not seg_metrics.supported(x, t, C)
        want, want_pred = host_counts(x, t)
        counts, pred = seg_metrics.seg_confusion_counts(x, t, C, return_preds=True)
        assert counts.dtype == torch.int32 and pred.dtype == torch.uint8
        assert np.array_equal(counts.cpu().numpy().astype(np.int64), want) and np.array_equal(pred.cpu().numpy(), want_pred)
        tracker = seg_metrics.SegMetricsTracker(C)
        tracker.update(x, t)
        assert np.abs(tracker.state.cpu().numpy() - host_state(want, x.shape[2] * x.shape[3])).max() <= ATOL


class _Stub(torch.nn.Module):
    """(B, nf, 3, H, W) -> (B * nf, C, H, W) through a 1 x 1 convolution: what eval_step needs of a model."""

    def __init__(self, C):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, C, 1)

    def forward(self, clip):
        return self.conv(clip.flatten(0, 1))


def test_eval_step_end_to_end(cuda, monkeypatch):
    from vivim_amd import seg_metrics, train_step as ts
    calls = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, P, stream: (calls.append(name), real_call(name, P, stream))[1])
    clip, onehot = ts.synthetic_batch(2, 3, 24, 3, cuda, seed=11)
    torch.manual_seed(12)
    model = _Stub(3).to(cuda)
    assert model.training
    with torch.no_grad():
        logits = model(clip)
    target = onehot.argmax(dim=2).view(6, 24, 24)
    want_loss = float(ts.recall_focused_loss(logits, target, 3))
    want_counts = host_counts(logits, target)[0]
    present = int(((want_counts[..., 0] + want_counts[..., 2]) > 0).sum())
    for fused in (False, True):
        tracker = seg_metrics.SegMetricsTracker(3)
        del calls[:]
        loss = ts.eval_step(model, clip, onehot, 3, tracker=tracker, amp_dtype=torch.float32, fused_loss=fused)
        assert calls == (["vivim_seg_loss_fwd"] if fused else []) + ["vivim_seg_metrics"]
        assert not model.training and not loss.requires_grad and loss.dim() == 0
        assert abs(float(loss) - want_loss) <= 1e-5 * abs(want_loss), (fused, float(loss), want_loss)
        res = tracker.get_results()
        assert sum(res["class_counts"]) == present
        assert np.abs(tracker.state.cpu().numpy() - host_state(want_counts, 24 * 24)).max() <= ATOL
        assert all(p.grad is None for p in model.parameters())
    loss = ts.eval_step(model, clip, onehot, 3, amp_dtype=torch.float32)             # no tracker: the loss alone
    assert abs(float(loss) - want_loss) <= 1e-5 * abs(want_loss)
