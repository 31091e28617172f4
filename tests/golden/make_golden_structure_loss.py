"""Writes tests/golden/structloss_*.npz: inputs, loss and d loss / d logits of the reference's own structure-loss functions on fp64
logits.  Not a test: run by hand where a checkout of the reference is at hand,
    python tests/golden/make_golden_structure_loss.py REFERENCE_DIR   (rewrites every structloss_* fixture deterministically)

The reference's training scripts do not import outside their own environment (pytorch_lightning, wandb, argv parsing at import), so
the generator takes the source text of just the two functions out of the files at generation time and executes it with torch and
F in scope; none of that text is kept.

    structloss_c3, structloss_c5    multiclass_structure_loss(logits, targets, C)       final_multiclass_training.py
    structloss_binary               structure_loss(pred, mask)                          complements/train_binary.py

The binary function spells the BCE keyword `reduce='none'`, which torch reads as the legacy flag reduce=True: as written it adds the
UNWEIGHTED mean BCE to the weighted IoU.  `loss` / `dlogits` of the binary fixture come from the function with that one keyword
spelled `reduction='none'` (the boundary-weighted BCE the multiclass function computes); `loss_as_written` / `dlogits_as_written`
come from the text exactly as it stands."""
import ast
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))


def _function(ref, path, name, edit=None):
    text = open(os.path.join(ref, path)).read()
    node = next(n for n in ast.walk(ast.parse(text)) if isinstance(n, ast.FunctionDef) and n.name == name)
    src = ast.get_source_segment(text, node)
    if edit:
        assert edit[0] in src
        src = src.replace(*edit)
    scope = {"torch": torch, "F": F}
    exec(compile(src, path, "exec"), scope)
    return scope[name]


def _grad(fn, logits, *args):
    x = logits.clone().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss = fn(x, *args)
    loss.backward()
    return loss.detach().numpy(), x.grad.numpy()


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit(__doc__)
    ref = sys.argv[1]
    multi = _function(ref, "final_multiclass_training.py", "multiclass_structure_loss")
    binary_as_written = _function(ref, "complements/train_binary.py", "structure_loss")
    binary = _function(ref, "complements/train_binary.py", "structure_loss", ("reduce='none'", "reduction='none'"))
    for name, (N, C, H, W), seed in (("c3", (2, 3, 33, 47), 1), ("c5", (1, 5, 40, 31), 2)):
        g = torch.Generator().manual_seed(seed)
        logits = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 4
        targets = torch.randint(0, C, (N, H, W), generator=g)
        targets[:, : H // 2, : W // 3] = 1                       # a solid region: windows that are full, empty and in between
        targets[0][targets[0] == C - 1] = 0                      # image 0 lacks the last class
        loss, grad = _grad(multi, logits, targets, C)
        np.savez_compressed(os.path.join(HERE, f"structloss_{name}.npz"), logits=logits.numpy(), targets=targets.numpy(), loss=loss,
                            dlogits=grad, eps=np.float64(1e-6))
        print(name, float(loss))
    N, C, H, W = 2, 1, 9, 11
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 4
    mask = (torch.rand(N, C, H, W, generator=g) < 0.4).double()
    loss, grad = _grad(binary, logits, mask)
    loss_w, grad_w = _grad(binary_as_written, logits, mask)
    np.savez_compressed(os.path.join(HERE, "structloss_binary.npz"), logits=logits.numpy(), mask=mask.numpy(), loss=loss, dlogits=grad,
                        loss_as_written=loss_w, dlogits_as_written=grad_w, eps=np.float64(1.0))
    print("binary", float(loss), "as written", float(loss_w))


if __name__ == "__main__":
    main()
