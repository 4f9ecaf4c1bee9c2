"""Host reference of the FP8 token index (include/polus_hip.h polus_fp8_quantize_rows): NumPy frexp for the exponent,
torch's CPU float8_e4m3fn cast for the rounding.  Per row x[0..E):

    amax = max |x_k| = m 2^k, m in [0.5, 1);   e = max(k - 9 + (m > 0.875), -100), e = 0 if amax == 0;
    scale = 2^e;   code_k = e4m3fn(x_k / 2^e), round to nearest even;   x ~ e4m3fn(code) * scale.

`mutate` plants one mistake, for the checks that the GPU tests' bitwise comparisons would see it."""
import numpy as np
import torch

EMIN = -100
FP8_MAX = 448.0


def decode(codes):
    """e4m3fn bytes -> float32 (exact)."""
    return torch.from_numpy(np.ascontiguousarray(codes, np.uint8)).view(torch.float8_e4m3fn).float().numpy()


def encode(values):
    """float32 -> e4m3fn bytes, round to nearest even (|values| <= 448)."""
    v = torch.from_numpy(np.ascontiguousarray(values, np.float32))
    return v.to(torch.float8_e4m3fn).view(torch.uint8).numpy()


_POS = decode(np.arange(0x7f, dtype=np.uint8))            # the 127 finite non-negative values, ascending


def encode_truncating(values):
    """The mutant: rounds toward zero."""
    v = np.ascontiguousarray(values, np.float32)
    mag = (np.searchsorted(_POS, np.abs(v), side="right") - 1).astype(np.uint8)
    return mag | (np.signbit(v).astype(np.uint8) << 7)


def exponent(x):
    """e [rows] (int) of the rule above."""
    amax = np.abs(np.asarray(x, np.float32)).max(-1)
    m, k = np.frexp(amax)
    e = np.maximum(k.astype(np.int64) - 9 + (m > 0.875), EMIN)
    return np.where(amax == 0, 0, e)


def quantize(x, mutate=None):
    """(codes uint8 [..., E], scale float32 [...], e int [...]) of float32 x (bf16 inputs: pass their f32 values)."""
    x = np.ascontiguousarray(x, np.float32)
    e = exponent(x)
    if mutate == "exponent+1":
        e = e + 1
    elif mutate == "exponent-1":
        e = e - 1
    scaled = np.ldexp(x, -e[..., None]).astype(np.float32)            # exact: a power of two
    if mutate == "truncate":
        codes = encode_truncating(scaled)
    else:
        codes = encode(np.clip(scaled, -FP8_MAX, FP8_MAX) if mutate == "exponent-1" else scaled)
    return codes, np.ldexp(np.float32(1), e).astype(np.float32), e


def dequantize(codes, scale):
    """float32 [..., E] = e4m3fn(codes) * scale (exact)."""
    return decode(codes) * np.asarray(scale, np.float32)[..., None]
