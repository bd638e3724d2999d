"""The error norms and the sequence mask that the case catalogues (tests/*_cases.py) and the GPU test modules share.  Three norms,
three names: each catalogue imports the one it means under its own public name (`from case_util import relerr_zero_exact as relerr`).
tests/test_gpu_guards_cpu.py holds each to its edge cases."""
import torch


def relerr(got, ref):
    """max |got - ref| / max |ref| in float64 over all elements, nothing masked out (NaN if anything is not finite)."""
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def relerr_zero_exact(got, ref, scale=None):
    """max |got - ref| / scale, scale = max |ref| unless given; an all-zero reference without a scale asks for exact zeros."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    n = float(ref.abs().max()) if scale is None else float(scale)
    if n == 0.0:
        return 0.0 if bool((got == 0).all()) else float("inf")
    return float((got - ref).abs().max() / n)


def relerr_floor(a, b):
    """max |a - b| / (max |b| + 1e-30) in the tensors' own dtype: finite on an all-zero b."""
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def seq_mask(lens, n):
    """[len(lens), n] fp32: 1 where position < length, 0 behind it."""
    return (torch.arange(n).unsqueeze(0) < torch.as_tensor(lens).unsqueeze(1)).float()
