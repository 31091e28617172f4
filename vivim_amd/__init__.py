"""vivim_amd -- MI355X-native (gfx950) implementation of Vivim's Temporal-Mamba-Block hot path:
causal_conv1d fwd/bwd + selective scan fwd/bwd as hand-written HIP kernels behind a C ABI
(include/vivim_hip.h), plus the host-side mirror of the reference's Python surface.

There is no CPU or PyTorch fallback: importing the op modules without the built
vivim_amd/csrc/libvivim_hip.so raises ImportError on first use.
"""
__version__ = "0.1.0"
from .generation import InferenceParams  # noqa: E402,F401  (a plain dataclass: importing it loads neither torch nor the library)


def __getattr__(name):
    # the validation metrics (seg_metrics.py) need torch: exported here, imported on first use
    if name in ("SegMetricsTracker", "seg_confusion_counts"):
        from . import seg_metrics
        return getattr(seg_metrics, name)
    if name in ("BinaryMetricsTracker", "binary_image_metrics"):      # the binary recipe's validation metrics (binary_metrics.py), likewise
        from . import binary_metrics
        return getattr(binary_metrics, name)
    if name == "bilinear_upsample":                    # the decode head's upsampling (upsample.py), likewise
        from . import upsample
        return upsample.bilinear_upsample
    if name in ("fused_decode_head", "fold_decode_head"):     # the eval-mode decode head (decode_head.py), likewise
        from . import decode_head
        return getattr(decode_head, name)
    if name == "upsample_concat":                      # the training decode head's upsample + dropout + concat (head_concat.py), likewise
        from . import head_concat
        return head_concat.upsample_concat
    if name in ("FusedStepAdamW", "lower_params", "raise_params"):   # the device-side clip + AdamW step (optimizer.py), likewise
        from . import optimizer
        return getattr(optimizer, name)
    # checkpoint, exact resume and the cosine schedule (checkpoint.py), likewise
    if name in ("CosineSchedule", "TrainState", "save_checkpoint", "load_checkpoint", "load_model_weights"):
        from . import checkpoint
        return getattr(checkpoint, name)
    # the structure loss (structure_loss.py), likewise.  `vivim_amd.structure_loss` itself is that module, so the eager binary
    # form is reached as vivim_amd.structure_loss.structure_loss
    if name in ("multiclass_structure_loss", "structure_loss_fused", "multiclass_structure_loss_fused"):
        from .structure_loss import multiclass_structure_loss, multiclass_structure_loss_fused, structure_loss_fused  # noqa: F401
        return locals()[name]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
