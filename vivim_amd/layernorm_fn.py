"""The reference's fused-norm surface (module path mamba_ssm/ops/triton/layernorm.py) over layernorm.py's token-major kernels:

    layer_norm_fn(x, weight, bias, residual=None, eps=1e-6, prenorm=False, residual_in_fp32=False, is_rms_norm=False)
    rms_norm_fn(x, weight, bias, residual=None, prenorm=False, residual_in_fp32=False, eps=1e-6)
    RMSNorm(hidden_size, eps=1e-5, device=None, dtype=None)

h = residual + x (or x), stored in residual's dtype (fp32 with residual_in_fp32 and no residual; x itself with neither), and
y = LayerNorm / RMSNorm of h AS STORED over the last dimension, in x's dtype; prenorm=True returns (y, h).  Two deliberate
differences from the reference: the statistics come from the stored sum, within one rounding of the residual
dtype of the reference's, and RMSNorm.forward calls rms_norm_fn with the arguments rms_norm_fn has.
CUDA rows the kernels take (layernorm.tm_add_supported) run them; CPU tensors, other dtype pairs and more than 1024 channels run
the same definition as a composition of torch ops."""
import torch

from . import layernorm as _ln


def _norm(h, weight, bias, eps, rms):
    h = h.float()
    if rms:
        y = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)
    else:
        d = h - h.mean(-1, keepdim=True)
        y = d * torch.rsqrt(d.pow(2).mean(-1, keepdim=True) + eps)
    if weight is not None:
        y = y * weight
    return y if bias is None else y + bias


def _composition(x, weight, bias, residual, eps, rms, res_dtype):
    h = x
    if residual is not None:
        h = (residual.float() + x.float()).to(res_dtype)
    elif res_dtype is not None and res_dtype != x.dtype:
        h = x.to(res_dtype)
    return h, _norm(h, weight, bias, eps, rms).to(x.dtype)


def layer_norm_fn(x, weight, bias, residual=None, eps=1e-6, prenorm=False, residual_in_fp32=False, is_rms_norm=False):
    if weight is not None and weight.dtype != torch.float32:
        weight = weight.float()                          # autograd casts the gradient back
    if bias is not None and bias.dtype != torch.float32:
        bias = bias.float()
    res_dtype = residual.dtype if residual is not None else (torch.float32 if residual_in_fp32 else None)
    if residual is not None:
        if _ln.tm_add_supported(residual, x, weight, bias) and weight is not None:
            h, y = _ln.add_layer_norm_tm(residual, x, weight, bias, eps, rms=is_rms_norm)
            return (y, h) if prenorm else y
    elif weight is not None and _ln.tm_add_supported(x, x, weight, bias):
        opened = res_dtype if res_dtype != x.dtype else None         # a stream opened in another dtype is a tensor of its own
        if opened is None or _ln.tm_add_pair_ok(x.dtype, opened):
            h, y = _ln.norm_tm_no_residual(x, weight, bias, eps, is_rms_norm, res_dtype=opened)
            return (y, x if h is None else h) if prenorm else y
    h, y = _composition(x, weight, bias, residual, eps, is_rms_norm, res_dtype)
    return (y, h) if prenorm else y


def rms_norm_fn(x, weight, bias, residual=None, prenorm=False, residual_in_fp32=False, eps=1e-6):
    return layer_norm_fn(x, weight, bias, residual, eps, prenorm, residual_in_fp32, True)


class RMSNorm(torch.nn.Module):
    def __init__(self, hidden_size, eps=1e-5, device=None, dtype=None):
        super().__init__()
        self.eps = eps
        self.weight = torch.nn.Parameter(torch.ones(hidden_size, device=device, dtype=dtype))
        self.register_parameter("bias", None)

    def reset_parameters(self):
        torch.nn.init.ones_(self.weight)

    def forward(self, x, residual=None, prenorm=False, residual_in_fp32=False):
        return rms_norm_fn(x, self.weight, self.bias, residual=residual, prenorm=prenorm, residual_in_fp32=residual_in_fp32,
                           eps=self.eps)
