"""What tests/test_abi_master_weights.py (CPU) and tests/test_gpu_master_weights.py (the kernels) share: the two input families
that exercise the 16-bit rounding of the master-weight step (csrc/optimizer.hip: p16 = RNE(master')), the expectation -- torch's
own cast -- and restatements of the kernel's two narrowing conversions that do not go through that cast.

    "subnormal": |p| log-uniform in [6e-8, 6e-5] -- fp16's subnormal range (its smallest subnormal is 5.96e-8, its smallest normal
                 6.10e-5): a conversion that flushes instead of rounding gives zeros here.  The exact halfway points between two
                 subnormals are mixed in: ties go to the even neighbour.
    "overflow":  |p| within +-48 of 65504, fp16's largest finite value: from 65520 on -- the tie included -- the result is inf.
For bf16 both families are ordinary normal numbers; they pin the integer rounding on many mantissa patterns, ties included."""
import numpy as np
import torch

FAMILIES = ("subnormal", "overflow")
N = 4096 + 37                                       # more than one map row, a tail that is no multiple of 4
DTYPES = (torch.float16, torch.bfloat16)


def family(name, seed=3, n=N):
    """-> n fp32 values of the family, both signs."""
    gen = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    if name == "subnormal":
        lo, hi = torch.log(torch.tensor(6e-8)), torch.log(torch.tensor(6e-5))
        mag = torch.exp(lo + (hi - lo) * torch.rand(n, generator=gen))
        k = torch.arange(1, 65, dtype=torch.float32)
        mag[:64] = (k + 0.5) * 2.0 ** -24             # halfway between subnormals k and k + 1 of fp16: exact in fp32
    else:
        mag = 65504.0 + 96.0 * (torch.rand(n, generator=gen) - 0.5)
        mag[:4] = torch.tensor([65504.0, 65519.996, 65520.0, 65536.0])      # the largest finite | just below the tie | the tie | above
    return (sign * mag).float()


def bits16(t):
    """A 16-bit tensor's bits, for comparisons in which a NaN equals itself and -0 differs from +0."""
    assert t.element_size() == 2
    return t.contiguous().view(torch.int16)


def narrow_bf16_restated(x):
    """opt_narrow<bf16> in torch integer arithmetic: (u + 0x7fff + bit 16 of u) >> 16, a NaN becomes 0x7fc0."""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    r = torch.where(torch.isnan(x), torch.full_like(r, 0x7FC0), r)
    return torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16)                # as two's-complement int16, like bits16


def narrow_f16_restated(x):
    """opt_narrow<fp16> is the hardware's IEEE conversion; numpy's is IEEE round-to-nearest-even in software."""
    with np.errstate(over="ignore"):                                              # overflow to inf is the point
        return torch.from_numpy(x.numpy().astype(np.float16).view(np.int16))
