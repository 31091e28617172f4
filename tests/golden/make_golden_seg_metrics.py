#!/usr/bin/env python3
"""Generate tests/golden/segm_*.npz from the reference's OWN validation metrics code.  Not a test; runs only where the reference
tree is present (the suite reads the committed .npz files).

The reference's `misc2.py` is loaded by path -- it imports `medpy` at module scope for its surface distances, which the tracker
never calls, so an empty stub module is registered under that name when the package is absent.  `MulticlassMetricsTracker` sits
in a training script that parses argv and imports Lightning at import time: its class node alone is taken out of the parsed
source (`ast`) and executed, with `np`, `torch` and `misc2` as its globals.  No reference text is written anywhere.

Every fixture: `logits` fp32 (N, C, H, W), drawn as randn and rounded to bf16 so that they are exact in fp32, fp16 and bf16 alike;
`targets` int64 (N, H, W); `calls` (K, 2), the image ranges of the successive update() calls; then what the reference returns:
`per_class` (6, C) fp64 in the order dice, jaccard, precision, recall, f_measure, specificity with NaN where it says None,
`mean` (6,), `class_counts` (C,), and `counts` (N, C, 3) = {tp, fp, fn} from its ConfusionMatrix on (argmax == c, gt == c).

Usage:  python tests/golden/make_golden_seg_metrics.py REFERENCE_DIR   (rewrites every segm_* fixture deterministically)"""
import ast
import importlib.util
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
METRICS = ("dice", "jaccard", "precision", "recall", "f_measure", "specificity")


def load_reference(ref):
    try:
        import medpy  # noqa: F401
    except ImportError:
        stub = types.ModuleType("medpy")
        stub.metric = types.ModuleType("medpy.metric")
        sys.modules["medpy"], sys.modules["medpy.metric"] = stub, stub.metric
    spec = importlib.util.spec_from_file_location("misc2", os.path.join(ref, "misc2.py"))
    misc2 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(misc2)
    path = os.path.join(ref, "final_multiclass_training.py")
    tree = ast.parse(open(path).read(), filename=path)
    node, = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "MulticlassMetricsTracker"]
    ns = {"np": np, "torch": torch, "misc2": misc2}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return misc2, ns["MulticlassMetricsTracker"]


def bf16_exact(t):
    return t.to(torch.bfloat16).to(torch.float32)


def save(name, misc2, Tracker, logits, targets, calls):
    N, C = logits.shape[:2]
    assert torch.equal(bf16_exact(logits), logits) and torch.equal(logits.to(torch.float16).float(), logits)
    tracker = Tracker(num_classes=C)
    for a, b in calls:
        tracker.update(logits[a:b], targets[a:b])
    res = tracker.get_results()
    per_class = np.array([[np.nan if v is None else float(v) for v in res[m]["per_class"]] for m in METRICS], dtype=np.float64)
    mean = np.array([float(res[m]["mean"]) for m in METRICS], dtype=np.float64)
    pred = logits.numpy().argmax(axis=1)
    gt = targets.numpy()
    counts = np.zeros((N, C, 3), dtype=np.int64)
    for n in range(N):
        for c in range(C):
            tp, fp, tn, fn = misc2.ConfusionMatrix((pred[n] == c).astype(np.int32), (gt[n] == c).astype(np.int32)).get_matrix()
            assert tp + fp + tn + fn == gt[n].size
            counts[n, c] = (tp, fp, fn)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), logits=logits.numpy(), targets=gt,
                        calls=np.array(calls, dtype=np.int64), per_class=per_class, mean=mean,
                        class_counts=np.array(res["class_counts"], dtype=np.int64), counts=counts)
    print(f"{name}: logits {tuple(logits.shape)}, class_counts {res['class_counts']}, "
          f"None in per_class: {int(np.isnan(per_class[0]).sum())}")
    return res, counts


def main(ref):
    misc2, Tracker = load_reference(ref)

    # ties (two rows of image 0 have all classes equal: first index), class 2 absent from image 1, image 2 all class 1 (the
    # specificity rule), one label that is no class, and a second update() call that repeats images 0-1
    g = torch.Generator().manual_seed(101)
    logits = bf16_exact(torch.randn(5, 3, 6, 7, generator=g))
    logits[0, :, 0:2, :] = logits[0, 0:1, 0:2, :]
    targets = torch.randint(0, 3, (5, 6, 7), generator=g)
    targets[1][targets[1] == 2] = 0
    targets[2] = 1
    targets[3, 2, 3] = 7
    assert (targets[0] == 2).any() and (targets[3] == 2).any() and (targets[4] == 2).any()
    res, counts = save("segm_c3_ties", misc2, Tracker, logits, targets, [(0, 5), (0, 2)])
    assert res["class_counts"] == [6, 7, 4] and counts[2, 1, 0] + counts[2, 1, 2] == 42

    g = torch.Generator().manual_seed(102)
    logits = bf16_exact(torch.randn(3, 2, 1, 1, generator=g))
    targets = torch.tensor([0, 1, 1]).view(3, 1, 1)
    save("segm_c2_1x1", misc2, Tracker, logits, targets, [(0, 3)])

    # classes 6 and 7 are in no image: None in per_class, left out of the mean
    g = torch.Generator().manual_seed(103)
    logits = bf16_exact(torch.randn(2, 8, 5, 13, generator=g))
    targets = torch.randint(0, 6, (2, 5, 13), generator=g)
    res, _ = save("segm_c8_odd", misc2, Tracker, logits, targets, [(0, 1), (1, 2)])
    assert res["class_counts"][6:] == [0, 0] and res["dice"]["per_class"][6] is None and min(res["class_counts"][:6]) > 0

    # class 1 is in the labels but never predicted (precision and F are 0 by rule); class 2 is predicted but in no label map
    g = torch.Generator().manual_seed(104)
    logits = torch.randn(4, 3, 5, 9, generator=g)
    logits[:, 1] -= 100.0
    logits = bf16_exact(logits)
    targets = torch.randint(0, 2, (4, 5, 9), generator=g)
    res, counts = save("segm_c3_unpredicted", misc2, Tracker, logits, targets, [(0, 4)])
    assert res["class_counts"] == [4, 4, 0] and res["precision"]["per_class"][1] == 0.0 and res["f_measure"]["per_class"][1] == 0.0
    assert counts[:, 2, 1].sum() > 0 and counts[:, 1, :2].sum() == 0


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "misc2.py")):
        sys.exit(__doc__)
    main(sys.argv[1])
