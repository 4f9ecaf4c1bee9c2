"""Cases of the FP8 token index tests (tests/test_fp8_index_cpu.py, tests/test_fp8_index_gpu.py)."""
import numpy as np

# (rows, E) of the quantiser tests: one row, rows that do not fill a workgroup of four waves, more than one workgroup
QUANT_SHAPES = [(1, 32), (5, 64), (67, 128), (9, 256)]
PLANTS = ("ties", "m=0.875", "m>0.875", "zero", "2^-30", "2^30")

# values that lie exactly half way between two neighbouring e4m3 codes once the row's scale is 1 (the row's maximum is
# 448 = 0.875 * 2^9, so e = 0); every one has at most 8 significant bits, so bf16 holds it
MIDPOINTS = np.array([17, -17, 19, -19, 21, 23, 1.0625, -1.0625, 1.1875, 2.0 ** -10, -2.0 ** -10, 3 * 2.0 ** -10,
                      5 * 2.0 ** -10, 432, -432, 400, 0.0166015625, 34, 38, -42, 136, 152, 2.125, 2.375], np.float32)
# what round-to-nearest-even makes of them
MIDPOINTS_RNE = np.array([16, -16, 20, -20, 20, 24, 1.0, -1.0, 1.25, 0.0, -0.0, 2.0 ** -8,
                          2.0 ** -8, 448, -448, 384, 0.015625, 32, 40, -40, 128, 160, 2.0, 2.5], np.float32)


def quant_rows(rows, E, mode, seed=0):
    """float32 [rows, E], N(0, 1), with the planted rows of PLANTS in rows 0 .. min(rows, 6) - 1 (in that order) and
    {plant: row}.  mode "bf16": the values are bf16 numbers already, so that rounding to bf16 keeps the plants."""
    import torch
    r = np.random.Generator(np.random.PCG64(9000 + 3 * seed + rows * 7 + E))
    x = r.standard_normal((rows, E)).astype(np.float32)
    if mode == "bf16":
        x = torch.as_tensor(x).to(torch.bfloat16).float().numpy()
    where = {}
    for p, name in enumerate(PLANTS[:min(rows, len(PLANTS))]):
        where[name] = p
        if name == "ties":
            x[p] = np.resize(MIDPOINTS, E)
            x[p, E - 1] = -448.0
        elif name in ("m=0.875", "m>0.875"):
            x[p] = np.clip(x[p], -1.5, 1.5)
            above = np.nextafter(np.float32(1.75), np.float32(2)) if mode == "f32" else np.float32(1.75 + 2.0 ** -7)
            x[p, 3] = -1.75 if name == "m=0.875" else above
        elif name == "zero":
            x[p] = 0.0
            x[p, 1] = -0.0
        elif name == "2^-30":
            x[p] = np.ldexp(x[p], -30)
        elif name == "2^30":
            x[p] = np.ldexp(x[p], 30)
    return x, where


# (Q, N, Lq, Ld, E) of the exact-integer test
INT_SHAPES = [(3, 40, 5, 17, 32), (4, 64, 31, 65, 64)]


def integer_case(shape, seed=0):
    """q [Q, Lq, E] integers in [-3, 3]; document code VALUES [N, Ld, E] integers in [-8, 8] (all of them e4m3
    numbers) and scales [N, Ld] from {1, 2, 4, 8}; ragged masks.  No two tokens of a document are equal or negated once
    scaled, so a kernel that takes a token's codes with another token's scale, or an operand in another order,
    changes a score.  Every dot product and score is an integer below 2^24: f32, bf16 x bf16 -> f32 and float64 agree
    exactly."""
    Q, N, Lq, Ld, E = shape
    r = np.random.Generator(np.random.PCG64(9500 + seed + Q + 3 * N + 5 * Lq + 7 * Ld + E))
    q = r.integers(-3, 4, size=(Q, Lq, E)).astype(np.float32)
    v = r.integers(-8, 9, size=(N, Ld, E)).astype(np.float32)
    s = (2.0 ** r.integers(0, 4, size=(N, Ld))).astype(np.float32)
    d = v * s[..., None]
    for c in range(N):
        both = np.concatenate([d[c], -d[c]])
        assert len(np.unique(both, axis=0)) == 2 * Ld, "a document holds equal or negated tokens"
    ql, dl = r.integers(1, Lq + 1, size=Q), r.integers(1, Ld + 1, size=N)
    qm = (np.arange(Lq)[None] < ql[:, None]).astype(np.int32)
    dm = (np.arange(Ld)[None] < dl[:, None]).astype(np.int32)
    dm[r.random((N, Ld)) < 0.15] = 0
    dm[:, 0] = 1
    dm[N - 1] = 0                                              # an empty document
    assert 3 * 8 * 8 * E * Lq < 2 ** 24
    return q, v, s, qm, dm
