"""Reference module path mamba_ssm/ops/triton/layernorm.py -> the HIP implementation."""
from vivim_amd.layernorm_fn import RMSNorm, layer_norm_fn, rms_norm_fn  # noqa: F401
