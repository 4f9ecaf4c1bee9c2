"""NumPy restatement of the residual codec of include/polus_hip.h (polus_residual_compress / polus_residual_decompress):
the four rules, residual, bucket by counting, packing, decode.  f32 arithmetic is numpy's float32; the bf16 rounding is
torch's CPU cast (round to nearest even).

`mutate=` plants one mistake, each the least visible of its kind, so that tests/test_residual_cpu.py can show that the
byte and bit comparisons of tests/test_residual_gpu.py would see it:
  "ge"        bucket by r >= cutoff (a residual ON a cutoff goes up)
  "msb"       most-significant-bit-first packing inside a byte
  "weights"   weights indexed off by one (bucket + 1, the top bucket wrapping)
  "round"     the centroid + weight sum formed in bf16 steps: the weight is rounded to bf16 before the addition"""
import numpy as np
import torch

MUTANTS = ("ge", "msb", "weights", "round")
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def to_mode(a, mode):
    """float32 array -> the float32 values of its round-to-nearest-even conversion to `mode`."""
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(DT[mode]).float().numpy()


def codes_u16(codes):
    return np.asarray(codes).astype(np.int64) & 0xFFFF


def buckets(x, codes, centroids, cutoffs, mutate=None):
    """uint8 [rows, E]: the bucket of every element (0 for rows whose code is >= K); x, centroids float32 holding
    values of the storage dtype."""
    x, centroids = np.asarray(x, np.float32), np.asarray(centroids, np.float32)
    cutoffs = np.asarray(cutoffs, np.float32)
    codes = codes_u16(codes)
    ok = codes < len(centroids)
    r = x - centroids[np.where(ok, codes, 0)]                 # one f32 subtraction
    b = np.zeros(r.shape, np.uint8)
    with np.errstate(invalid="ignore"):
        for c in cutoffs:                                     # counting: a NaN residual is above no cutoff
            b += (r >= c) if mutate == "ge" else (r > c)
    b[~ok] = 0
    return b


def pack(b, nbits, mutate=None):
    """uint8 [rows, E * nbits / 8]: element k in byte k * nbits / 8 at bits [nbits * (k mod 8 / nbits), +nbits)."""
    rows, E = b.shape
    per = 8 // nbits
    b = b.reshape(rows, E // per, per).astype(np.uint8)
    pos = np.arange(per)
    shift = (nbits * (per - 1 - pos if mutate == "msb" else pos)).astype(np.uint8)
    return np.bitwise_or.reduce(b << shift, axis=-1)


def unpack(packed, nbits, mutate=None):
    rows, nb = packed.shape
    per = 8 // nbits
    pos = np.arange(per)
    shift = nbits * (per - 1 - pos if mutate == "msb" else pos)
    return ((packed[..., None].astype(np.uint32) >> shift) & ((1 << nbits) - 1)).reshape(rows, nb * per).astype(np.int64)


def compress(x, codes, centroids, cutoffs, nbits, mutate=None):
    return pack(buckets(x, codes, centroids, cutoffs, mutate), nbits, mutate)


def decompress(codes, packed, centroids, weights, nbits, mode, mutate=None):
    """float32 [rows, E] holding values of `mode`: T(f32(centroid) + weights[bucket]); zeros for codes >= K."""
    centroids, weights = np.asarray(centroids, np.float32), np.asarray(weights, np.float32)
    codes = codes_u16(codes)
    ok = codes < len(centroids)
    b = unpack(np.asarray(packed), nbits, mutate)
    if mutate == "weights":
        b = (b + 1) % len(weights)
    w = weights[b]
    if mutate == "round":
        w = to_mode(w, "bf16")
    y = to_mode(centroids[np.where(ok, codes, 0)] + w, mode)                  # one f32 addition, one rounding
    return np.where(ok[:, None], y, np.float32(0.0)).astype(np.float32)


def fit_tables(residuals, nbits):
    """(cutoffs, weights) f32: the (j + 1) / 2^nbits and (b + 1/2) / 2^nbits quantiles of all residual elements,
    numpy.quantile in float64 with method="linear"."""
    n = 1 << nbits
    flat = np.asarray(residuals, np.float32).astype(np.float64).ravel()
    return (np.quantile(flat, np.arange(1, n) / n, method="linear").astype(np.float32),
            np.quantile(flat, (np.arange(n) + 0.5) / n, method="linear").astype(np.float32))


def sample_slots(seed, N, Ld, mask, sample):
    """The token slots CorpusIndex.fit_centroids and fit_codec draw: seed, N, Ld and the masks only."""
    S = N * Ld
    r = np.random.Generator(np.random.PCG64(int(seed)))
    slots = r.permutation(S) if S <= int(sample) else r.choice(S, size=int(sample), replace=False)
    return slots[np.asarray(mask).reshape(-1)[slots] != 0]
