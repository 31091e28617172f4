"""GPU: vivim_amd.binary_metrics (csrc/binary_metrics.hip) against the definition restated in numpy fp64
(binary_metrics_cases.restate64) and against the fixtures written by the reference's own classes.

Bounds, none of them measured on the code under test:
  histograms and per-threshold counts   exactly
  the six sweep metrics, E-measure      1e-12 absolute: fp64 arithmetic on the same integers, and the order of a sum of 256 terms in
                                        [0, 1] costs at most 256 * 2^-53
  MAE                                   H W 2^-53 absolute: an fp64 sum of H W terms in [0, 1] in any order
  S-measure                             1e-12 + 64 |restate64 - restate_exact| per image, computed here on the CPU: the distance
                                        between a plain and an exactly summed evaluation says how ill-conditioned that image is
The worst figures go to the parity log that conftest.py keeps."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import binary_metrics_cases as bc
from conftest import _PARITY_LOG, DT, ROOT

pytestmark = pytest.mark.gpu

FIXTURES = bc.fixtures()
GT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16, "uint8": torch.uint8, "bool": torch.bool}
SWEEP_AND_E = [0, 1, 2, 3, 4, 5, 7]
# every fixture in every pred dtype that holds its values exactly, with every mask dtype
GRID = [(name, pd, gd) for name in sorted(FIXTURES) for pd in DT if pd == "fp32" or int(FIXTURES[name]["all_dtypes"]) for gd in GT]
_REF = {}


def _log(what, dtype, figures):
    text = "\t".join(f"{k}={v:.3e}" for k, v in figures.items())
    try:
        os.makedirs(os.path.dirname(_PARITY_LOG), exist_ok=True)
        with open(_PARITY_LOG, "a") as f:
            f.write(f"test_gpu_binary_metrics\t{what}\t{dtype}\t{text}\n")
    except OSError:
        pass
    print(f"binary_metrics {what} {dtype}: {text}")


def reference(key, pred, gt):
    """restate64 and restate_exact per image, computed once per input set `key` and shared."""
    if key not in _REF:
        _REF[key] = [(bc.restate64(pred[n], gt[n]), bc.restate_exact(pred[n], gt[n])) for n in range(pred.shape[0])]
    return _REF[key]


def check(what, key, pred_np, gt_np, values, hist, dtype="fp32"):
    """`values` (N, 9) and `hist` (N, 4, 256) of the kernels against the definition; -> the worst figures."""
    values, hist = values.cpu().numpy(), hist.cpu().numpy()
    N, H, W = pred_np.shape
    assert values.shape == (N, 9) and values.dtype == np.float64 and hist.shape == (N, 4, 256) and hist.dtype == np.int32
    worst = {"sweep_E": 0.0, "MAE": 0.0, "MAE_bound": H * W * 2.0 ** -53, "S": 0.0, "S_over_bound": 0.0}
    for n, (r, x) in enumerate(reference(key, pred_np, gt_np)):
        assert np.array_equal(hist[n, 0], r["sweep_fg"]) and np.array_equal(hist[n, 1], r["sweep_bg"]), (what, n)
        assert np.array_equal(hist[n, 2], r["e_fg"]) and np.array_equal(hist[n, 3], r["e_bg"]), (what, n)
        counts = bc.counts_from_hist(hist[n], int(gt_np[n].sum()), H * W)[0]
        assert np.array_equal(counts, r["counts"]), (what, n)
        err = np.abs(values[n] - r["values"])
        print(f"{what} image {n}: |err| {err.tolist()}")
        s_bound = 1e-12 + 64 * abs(r["values"][6] - x["values"][6])
        worst["sweep_E"], worst["MAE"], worst["S"] = max(worst["sweep_E"], err[SWEEP_AND_E].max()), max(worst["MAE"], err[8]), max(worst["S"], err[6])
        worst["S_over_bound"] = max(worst["S_over_bound"], err[6] / s_bound)
        assert err[SWEEP_AND_E].max() <= 1e-12, (what, n, err)
        assert err[8] <= H * W * 2.0 ** -53, (what, n, err[8])
        assert err[6] <= s_bound, (what, n, err[6], s_bound)
    _log(what, dtype, worst)
    return worst


def run(pred, gt):
    from vivim_amd import binary_metrics as bm
    assert bm.supported(pred, gt)
    values, hist = bm.binary_image_metrics(pred, gt, return_hist=True)
    assert values.device == pred.device and torch.equal(bm.binary_image_metrics(pred, gt), values)          # without the histograms
    return values, hist


@pytest.mark.parametrize("name,pd,gd", GRID)
def test_fixtures(cuda, name, pd, gd):
    f = FIXTURES[name]
    pred_np, gt_np = f["pred"], f["gt"] != 0
    pred, gt = torch.from_numpy(pred_np).to(DT[pd]).to(cuda), torch.from_numpy(f["gt"]).to(GT[gd]).to(cuda)
    assert torch.equal(pred.float().cpu(), torch.from_numpy(pred_np))
    values, hist = run(pred, gt)
    check(f"fixture {name} gt {gd}", name, pred_np, gt_np, values, hist, pd)
    hist = hist.cpu().numpy()
    for n in range(pred_np.shape[0]):            # and the reference's own numbers: integers exactly, sweep and E to 1e-12
        counts, e_fg, e_bg = bc.counts_from_hist(hist[n], int(gt_np[n].sum()), gt_np[n].size)
        assert np.array_equal(counts, f["counts"][n]) and np.array_equal(e_fg, f["e_fg"][n]) and np.array_equal(e_bg, f["e_bg"][n])
        err = np.abs(values[n].cpu().numpy() - f["values"][n])
        assert err[SWEEP_AND_E].max() <= 1e-12
        assert err[6] <= 4 * bc.REFERENCE_FP32_GAP["Smeasure"] and err[8] <= 4 * bc.REFERENCE_FP32_GAP["MAE"]


def _generated(shape, n, seed):
    key = ("generated", shape, n, seed)
    if key not in _REF:
        _REF[key] = bc.make_inputs(shape, n, seed)
    return key, _REF[key]


@pytest.mark.parametrize("pd", list(DT))
def test_five_images_of_more_than_one_block(cuda, pd):
    """(33, 70): 2310 pixels are three workgroups of fp32 and two of a 16-bit type, the last one partly filled."""
    key, (pred_np, gt_np) = _generated((33, 70), 5, 11)
    values, hist = run(torch.from_numpy(pred_np).to(DT[pd]).to(cuda), torch.from_numpy(gt_np).to(cuda))
    check("five images (33, 70)", ("ref",) + key, pred_np, gt_np, values, hist, pd)


def test_the_grid_stride_loop(cuda):
    """(256, 256) fp32: 64 blocks' worth of pixels on 32 workgroups."""
    key, (pred_np, gt_np) = _generated((256, 256), 1, 12)
    values, hist = run(torch.from_numpy(pred_np).to(cuda), torch.from_numpy(gt_np).to(torch.uint8).to(cuda))
    check("one image (256, 256)", ("ref",) + key, pred_np, gt_np, values, hist)


@pytest.mark.parametrize("pd", list(DT))
def test_views_that_forbid_vector_loads(cuda, pd):
    """A view one element into its storage (no 16-byte alignment), and a batch stride wider than the image and odd."""
    key, (pred_np, gt_np) = _generated((33, 70), 5, 11)
    N, H, W = pred_np.shape
    want, want_hist = run(torch.from_numpy(pred_np).to(DT[pd]).to(cuda), torch.from_numpy(gt_np).to(cuda))
    flat_p, flat_g = torch.zeros(N * H * W + 1, dtype=DT[pd], device=cuda), torch.zeros(N * H * W + 1, dtype=torch.float32, device=cuda)
    pred, gt = flat_p[1:].view(N, H, W), flat_g[1:].view(N, H, W)
    pred.copy_(torch.from_numpy(pred_np))
    gt.copy_(torch.from_numpy(gt_np))
    assert pred.data_ptr() % 16 != 0 and gt.data_ptr() % 16 != 0
    values, hist = run(pred, gt)
    check("offset view", ("ref",) + key, pred_np, gt_np, values, hist, pd)
    assert torch.equal(values, want) and torch.equal(hist, want_hist)              # the same pixels per thread: the same bits
    wide_p = torch.full((N, H * W + 5), float("nan"), dtype=DT[pd], device=cuda).as_strided((N, H, W), (H * W + 5, W, 1))
    wide_g = torch.full((N, H * W + 3), 1, dtype=torch.uint8, device=cuda).as_strided((N, H, W), (H * W + 3, W, 1))
    wide_p.copy_(torch.from_numpy(pred_np))
    wide_g.copy_(torch.from_numpy(gt_np))
    values, hist = run(wide_p, wide_g)
    check("wide batch stride", ("ref",) + key, pred_np, gt_np, values, hist, pd)
    assert torch.equal(values, want) and torch.equal(hist, want_hist)


def test_the_constant_quadrant_takes_the_one_branch(cuda):
    pred_np, gt_np = bc.constant_quadrant()
    values, hist = run(torch.from_numpy(pred_np).to(cuda), torch.from_numpy(gt_np).to(cuda))
    check("constant quadrant", "constant_quadrant", pred_np, gt_np, values, hist)
    wrong = reference("constant_quadrant", pred_np, gt_np)[0][0]["values"][6] - 0.5 * (33 * 17) / (33 * 70)
    assert abs(values[0, 6].item() - wrong) > 0.1


def test_accumulation_repeats_and_streams(cuda):
    from vivim_amd import binary_metrics as bm
    key, (pred_np, gt_np) = _generated((33, 70), 5, 11)
    pred, gt = torch.from_numpy(pred_np).to(cuda), torch.from_numpy(gt_np).to(cuda)
    one, two, again, five = (bm.BinaryMetricsTracker() for _ in range(4))
    one.update(pred, gt)
    two.update(pred[:2], gt[:2])
    two.update(pred[:0], gt[:0])                                                       # an empty batch: nothing
    two.update(pred[2:], gt[2:])
    again.update(pred, gt)
    assert one.state.device == pred.device and one.state.dtype == torch.float64 and one.state.shape == (10,)
    assert torch.equal(one.state, two.state) and torch.equal(one.state, again.state)  # the same images: the same bits
    five.update(pred[:4].view(2, 2, 1, 33, 70), gt[:4].view(2, 2, 1, 33, 70))
    five.update(pred[4:, None], gt[4:, None])
    assert torch.equal(one.state, five.state)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    on_side = bm.BinaryMetricsTracker()
    with torch.cuda.stream(side):
        on_side.update(pred[:2], gt[:2])
        on_side.update(pred[2:], gt[2:])
    side.synchronize()
    torch.cuda.current_stream(cuda).wait_stream(side)
    assert torch.equal(one.state, on_side.state)
    values = bm.binary_image_metrics(pred, gt)
    want = torch.zeros(10, dtype=torch.float64)
    for n in range(5):
        want[:9] += values[n].cpu()
    want[9] = 5
    assert torch.equal(one.state.cpu(), want)                                         # added in image order
    res = one.get_results()
    assert list(res) == list(bc.VALUES) and all(res[k] == want[i].item() / 5 for i, k in enumerate(bc.VALUES))
    ref = np.stack([r["values"] for r, _ in reference(("ref",) + key, pred_np, gt_np)]).mean(0)
    assert max(abs(res[k] - ref[i]) for i, k in enumerate(bc.VALUES)) <= 1e-9
    one.reset()
    assert not bool(one.state.any())


def test_update_neither_synchronises_nor_copies_to_the_host(cuda):
    from vivim_amd import binary_metrics as bm
    key, (pred_np, gt_np) = _generated((33, 70), 5, 11)
    pred, gt = torch.from_numpy(pred_np).to(torch.bfloat16).to(cuda), torch.from_numpy(gt_np).to(cuda)
    want = bm.binary_image_metrics(pred, gt)                                           # the library is loaded, the thresholds are there
    tracker = bm.BinaryMetricsTracker()
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tracker.update(pred, gt)                                                       # the first one also makes the state
        tracker.update(pred.view(1, 5, 1, 33, 70), gt.view(1, 5, 1, 33, 70))
        values = bm.binary_image_metrics(pred, gt)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert torch.equal(values, want) and tracker.state[9].item() == 10.0


def test_where_the_kernels_do_not_apply_the_eager_definition_runs(cuda):
    from vivim_amd import binary_metrics as bm
    key, (pred_np, gt_np) = _generated((33, 70), 5, 11)
    pred, gt = torch.from_numpy(pred_np).to(cuda), torch.from_numpy(gt_np).to(cuda)
    turned = pred.transpose(1, 2).contiguous().transpose(1, 2)                        # rows not contiguous
    assert not bm.supported(turned, gt) and not bm.supported(pred.double(), gt) and not bm.supported(pred, gt.cpu())
    assert not bm.supported(pred, gt.long())
    values, hist = bm.binary_image_metrics(turned, gt, return_hist=True)
    check("eager on the device", ("ref",) + key, pred_np, gt_np, values, hist)
    a, b = bm.BinaryMetricsTracker(), bm.BinaryMetricsTracker()
    a.update(turned, gt)
    b.update(pred, gt)
    assert a.state.device == pred.device and (a.state - b.state).abs().max().item() <= 1e-10


CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, "tests")
import binary_metrics_cases as bc
from vivim_amd import _lib
from vivim_amd import binary_metrics as bm
assert _lib.GUARD
dev = torch.device("cuda:0")
n = 0
for shape, count, dt in (((33, 70), 5, torch.float32), ((5, 7), 3, torch.bfloat16), ((1, 2), 2, torch.float16), ((97, 131), 1, torch.float32)):
    pred, gt = bc.make_inputs(shape, count, 31) if shape != (1, 2) else (np.array([[[0.25, 0.75]]] * 2, dtype=np.float32), np.array([[[0, 1]], [[1, 1]]], dtype=bool))
    pred, gt = torch.from_numpy(pred).to(dt).to(dev), torch.from_numpy(gt).to(dev)
    values, hist = bm.binary_image_metrics(pred, gt, return_hist=True)      # check_guards runs after the launch
    tracker = bm.BinaryMetricsTracker()
    tracker.state = _lib.empty((10,), torch.float64, dev).zero_()
    tracker._fresh = False
    tracker.update(pred, gt)
    _lib.check_guards("state")
    assert torch.isfinite(values).all() and tracker.state[9].item() == count
    n += 1
print("GUARD_OK", n)
"""


def test_writes_stay_inside_their_buffers_under_guard(cuda):
    env = dict(os.environ, VIVIM_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GUARD_OK 4" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
