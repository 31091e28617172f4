"""Reference module path mamba_ssm/utils/generation.py: only the cache handle is built (the sampling loop and the
language-model glue are outside this package)."""
from vivim_amd.generation import InferenceParams  # noqa: F401
