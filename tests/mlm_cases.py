"""Cases of the masked-LM kernel tests, shared by test_mlm_cpu.py (tolerance meta-test) and test_mlm_gpu.py.

Wide loss: six rows per case --
  0  label -1 (ignored)                     1  label -100 (ignored)
  2  label V - 1, the row's maximum in the LAST column, by a margin of at least 0.5
  3  label 0, the row's maximum in the last element of a 16-byte chunk (where the row holds a whole chunk)
  4  label V + 3 (rejected: ignored and counted in stats[1])
  5  label V // 2, entries near +-1e4: most exponentials underflow
Rows 0-4 are N(0, scale).  The bounds: loss at TOL[float32] (the arithmetic is f32 for both dtypes), f32 dlogits at
elem_err(1e-4, 1e-6), bf16 dlogits at the same floor with rtol 2^-8 (half an ulp of bf16 storage on the f32 error)."""
import functools

import numpy as np

STAGE_BYTES = 128 * 1024                 # polus_amd/csrc/xent_wide.hip XW_STAGE_BYTES: wider rows stream
ESIZE = {"f32": 4, "bf16": 2}
WIDTHS = {dt: (1, 7, 8, 257, 2049, 30522, STAGE_BYTES // es + 1) for dt, es in ESIZE.items()}
SCALES = (1.0, 12.0)
LABEL_ROWS = 6
DL_RTOL = {"f32": 1e-4, "bf16": 2.0 ** -8}
DL_FLOOR = 1e-6


def labels_for(V):
    return np.array([-1, -100, V - 1, 0, V + 3, V // 2], np.int32)


@functools.lru_cache(maxsize=None)
def logits_for(V, scale, dtype="f32"):
    """[6, V] float64, before rounding to the storage dtype."""
    rng = np.random.Generator(np.random.PCG64(1000 + V))
    x = rng.standard_normal((LABEL_ROWS, V)) * scale
    x[2, V - 1] = x[2].max() + 1.0                              # >= 0.5 after bf16 rounding too: |x| < 64 there, ulp <= 0.25
    E = 16 // ESIZE[dtype]
    if V >= E:
        x[3, (V // E) * E - 1] = x[3].max() + 1.0
    sign = np.where(rng.random(V) < 0.5, -1.0, 1.0)
    x[5] = sign * 1e4 + rng.standard_normal(V)
    x.setflags(write=False)
    return x


def padded_ld(V, dtype):
    """A row stride of whole 16-byte chunks with at least one padding column."""
    E = 16 // ESIZE[dtype]
    return (V // E + 1) * E


def expected_route(V, ld, dtype):
    """(path, vec16) for a 16-byte aligned base."""
    es = ESIZE[dtype]
    return ("staged" if V * es <= STAGE_BYTES else "streaming"), (ld * es) % 16 == 0


def wide_cases():
    return [(dt, V, pad, inplace, scale) for dt in ("f32", "bf16") for V in WIDTHS[dt] for pad in (False, True)
            for inplace in (False, True) for scale in SCALES]


def wide_id(c):
    dt, V, pad, inplace, scale = c
    return f"{dt}-V{V}-{'pad' if pad else 'tight'}-{'inplace' if inplace else 'out'}-s{scale:g}"


# gather / scatter: T rows, index list with -1, a repeat, row 0 and row T - 1
GATHER_T = 37
GATHER_IDX = np.array([5, -1, 0, 36, 17, 5, 22, -1, 36, 9, 40], np.int32)       # 40 >= T: a zero row as well
GATHER_SHAPES = ((8, 8, 0), (64, 64, 0), (768, 768, 0), (772, 772, 0), (8, 12, 1))   # (H, row stride, base offset in elements)
