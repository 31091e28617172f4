#!/usr/bin/env python3
"""Generate tests/golden/binm_*.npz from the reference's OWN binary validation metrics.  Not a test; runs only where the reference
tree is present (the suite reads the committed .npz files).

The reference's `poloy_metrics.py` (Smeasure, Emeasure, MAE) and `misc2.py` (the six confusion metrics) are loaded by path;
`misc2` imports `medpy` at module scope for surface distances that nothing here calls, so an empty stub module is registered under
that name when the package is absent.  The loop of its `on_validation_epoch_end` (complements/train_binary.py:205-282) is followed
call by call: the three classes step on the fp32 map and the float mask, then 256 thresholds of numpy.linspace(1, 0, 256) are
compared with the map as a torch tensor and each binarised map goes through misc2.  No reference text is written anywhere.

Every fixture: `pred` fp32 (N, H, W); `gt` uint8 (N, H, W); `values` fp64 (N, 9) in the order Dice, Jaccard, Precision, Recall,
Fmeasure, specificity, Smeasure, Emeasure, MAE as the reference returns them per image; `counts` int64 (N, 256, 4) = tp, fp, fn, tn
of its ConfusionMatrix per threshold; `e_fg`, `e_bg` int64 (N, 256), the two histograms of its cal_em_with_cumsumhistogram;
`all_dtypes` (0 / 1): whether every value of `pred` is exact in bf16 and fp16 as well.

Usage:  python tests/golden/make_golden_binary_metrics.py REFERENCE_DIR   (rewrites every binm_* fixture deterministically)"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import binary_metrics_cases as cases  # noqa: E402


def load_reference(ref):
    try:
        import medpy  # noqa: F401
    except ImportError:
        stub = types.ModuleType("medpy")
        stub.metric = types.ModuleType("medpy.metric")
        sys.modules["medpy"], sys.modules["medpy.metric"] = stub, stub.metric
    mods = []
    for name in ("misc2", "poloy_metrics"):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


def reference_image(misc2, pm, pred, gt):
    """One image as the reference's validation loop treats it: pred fp32 (H, W), gt float32 (H, W) of zeros and ones."""
    sm, em, mae = pm.Smeasure(), pm.Emeasure(), pm.MAE()
    sm.step(pred, gt)
    em.step(pred, gt)
    mae.step(pred, gt)
    bins = np.linspace(0, 256, 257)
    pn, g = pm._prepare_data(pred, gt)
    e = (pn * 255).astype(np.uint8)
    e_fg, e_bg = np.histogram(e[g], bins=bins)[0], np.histogram(e[~g], bins=bins)[0]
    pred_t, gt_t = torch.from_numpy(pred), torch.from_numpy(gt)
    gt_i = (gt_t > 0.5).to(int).numpy()
    lists = [[] for _ in range(6)]
    counts = np.zeros((256, 4), dtype=np.int64)
    for j, threshold in enumerate(np.linspace(1, 0, 256)):
        test = (pred_t > threshold).to(int).numpy()
        for k, fn in enumerate((misc2.dice, misc2.jaccard, misc2.precision, misc2.recall, misc2.fscore, misc2.specificity)):
            lists[k].append(fn(test, gt_i))
        tp, fp, tn, fn_ = misc2.ConfusionMatrix(test, gt_i).get_matrix()
        counts[j] = (tp, fp, fn_, tn)
    six = [sum(v) / len(v) for v in lists]
    values = np.array(six + [float(sm.sms[-1]), float(np.mean(em.changeable_ems[-1])), float(mae.maes[-1])], dtype=np.float64)
    return values, counts, e_fg.astype(np.int64), e_bg.astype(np.int64)


GAP = {"MAE": 0.0, "Smeasure": 0.0}


def save(name, mods, pred, gt, all_dtypes):
    pred, gt = np.ascontiguousarray(pred, dtype=np.float32), np.ascontiguousarray(gt).astype(np.uint8)
    if all_dtypes:
        t = torch.from_numpy(pred)
        assert torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.to(torch.float16).float(), t), name
    res = [reference_image(*mods, pred[n], gt[n].astype(np.float32)) for n in range(pred.shape[0])]
    values, counts, e_fg, e_bg = (np.stack([r[k] for r in res]) for k in range(4))
    assert np.isfinite(values).all(), name
    for n in range(pred.shape[0]):
        mine = cases.restate64(pred[n], gt[n] != 0)
        assert np.array_equal(mine["counts"], counts[n]) and np.array_equal(mine["e_fg"], e_fg[n]) and np.array_equal(mine["e_bg"], e_bg[n]), name
        assert np.abs(mine["values"][[0, 1, 2, 3, 4, 5, 7]] - values[n][[0, 1, 2, 3, 4, 5, 7]]).max() <= 1e-12, name
        GAP["Smeasure"] = max(GAP["Smeasure"], abs(mine["values"][6] - values[n][6]))
        GAP["MAE"] = max(GAP["MAE"], abs(mine["values"][8] - values[n][8]))
    path = os.path.join(OUT, f"binm_{name}.npz")
    np.savez_compressed(path, pred=pred, gt=gt, values=values, counts=counts, e_fg=e_fg, e_bg=e_bg, all_dtypes=np.int64(all_dtypes))
    print(f"binm_{name}: pred {pred.shape}, {os.path.getsize(path)} bytes, Smeasure {np.round(values[:, 6], 4).tolist()}")


def main(ref):
    mods = load_reference(ref)
    warnings.simplefilter("ignore")                       # the reference divides by zero where its result is NaN

    # probability maps and binarised maps, values exact in every pred dtype
    for k, (shape, n) in enumerate((((5, 7), 3), ((33, 70), 2), ((64, 64), 2), ((97, 131), 1))):
        pred, gt = cases.make_inputs(shape, n, 200 + k)
        save(f"prob_{shape[0]}x{shape[1]}", mods, pred, gt, 1)
        pred, gt = cases.make_inputs(shape, n, 300 + k, binarised=True)
        save(f"bin_{shape[0]}x{shape[1]}", mods, pred, gt, 1)

    # two pixels: every S-measure branch that needs fewer ends in the NaN rule (G == 1, S - G == 1) or in the empty / full mask
    pred = np.array([[[0.25, 0.75]], [[0.25, 0.75]], [[0.25, 0.75]], [[0.5, 0.5]], [[1.0, 0.0]]], dtype=np.float32)
    gt = np.array([[[0, 1]], [[1, 1]], [[0, 0]], [[1, 0]], [[1, 0]]], dtype=bool)
    save("1x2", mods, pred, gt, 1)

    # the edge cases on one shape: an empty mask, a full mask, a constant prediction (mx == mn), a mask confined to the last
    # column (X == W: two empty quadrants, S-measure 0), G == 1, S - G == 1
    rng = np.random.default_rng(401)
    base, blob = cases.make_inputs((33, 70), 6, 402)
    gt = blob.copy()
    gt[0] = False
    gt[1] = True
    base[2] = 0.5
    gt[3] = False
    gt[3, 4:20, -1] = True
    gt[4] = False
    gt[4, 11, 23] = True
    gt[5] = True
    gt[5, 30, 2] = False
    save("edges_33x70", mods, base, gt, 1)

    # a prediction made of fp32-rounded thresholds themselves: the strict `>`.  Exact in fp32 only.
    pred = cases.THRESHOLDS[rng.integers(0, 256, size=(2, 33, 70))]
    save("thresholds_33x70", mods, pred, cases.blob_mask(rng, 2, 33, 70), 0)

    print("largest |reference - restate64|:", GAP)


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "poloy_metrics.py")):
        sys.exit(__doc__)
    main(sys.argv[1])
