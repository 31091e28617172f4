"""The decode-time cache handle `Mamba.forward(inference_params=...)` takes: the fields of the reference's
mamba_ssm/utils/generation.py:18-27 that the module reads.  Any object with `seqlen_offset` and
`key_value_memory_dict` works in its place."""
from dataclasses import dataclass, field


@dataclass
class InferenceParams:
    max_seqlen: int
    max_batch_size: int
    seqlen_offset: int = 0
    key_value_memory_dict: dict = field(default_factory=dict)

    def reset(self, max_seqlen, max_batch_size):
        self.max_seqlen = max_seqlen
        self.max_batch_size = max_batch_size
        self.seqlen_offset = 0
