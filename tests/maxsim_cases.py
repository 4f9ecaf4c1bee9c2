"""Cases and tolerances of the MaxSim kernel tests (tests/test_maxsim_gpu.py); tests/test_maxsim_cpu.py checks
that every tolerance sits at least 5x below the score change of a single wrong decision of the kernel."""
import numpy as np

# (B, k, Lq, Ld, E): B queries, N = (1 + k) B documents
SHAPES = [(1, 0, 1, 1, 32), (3, 0, 5, 17, 32), (4, 2, 31, 65, 64), (8, 1, 32, 180, 128), (5, 1, 33, 256, 128),
          (2, 0, 64, 512, 256)]
BENCH = (64, 1, 32, 256, 128)                     # the ColBERT batch of tools/maxsim_bench.py (bf16 only)
MASKS = ["none", "ones", "ragged"]

# relative to max|reference| over the tensor (tests/util.relerr); set at 2-3x the worst error measured on one
# MI355X over SHAPES x MASKS (+ BENCH in bf16): score 2.6e-7 (f32) / 2.0e-7 (bf16), dQ and dD 3.1e-7 (f32) /
# 3.0e-3 (bf16).  Scores: the reference runs on the inputs as the device sees them (bf16: rounded), so both engines
# differ from it only by f32 accumulation; gradients: bf16 rounds dQ / dD once.
TOL = {"f32": dict(score=6e-7, grad=8e-7, norm=1e-6),
       "bf16": dict(score=5e-7, grad=8e-3, norm=8e-3)}


def make_case(shape, masks, seed=0):
    """q [B, Lq, E], d [N, Ld, E] (float32, N(0, 1)), qmask [B, Lq] / dmask [N, Ld] int32 or None."""
    B, k, Lq, Ld, E = shape
    N = (1 + k) * B
    r = np.random.Generator(np.random.PCG64(1000 + 7 * seed + B * 31 + Lq * 17 + Ld * 5 + E))
    q = r.standard_normal((B, Lq, E)).astype(np.float32)
    d = r.standard_normal((N, Ld, E)).astype(np.float32)
    if masks == "none":
        return q, d, None, None
    if masks == "ones":
        return q, d, np.ones((B, Lq), np.int32), np.ones((N, Ld), np.int32)
    # ragged prefix lengths (1 among them), holes, one document and one query without a valid token
    ql = r.integers(1, Lq + 1, size=B)
    dl = r.integers(1, Ld + 1, size=N)
    ql[0], dl[0] = 1, 1
    qm = (np.arange(Lq)[None] < ql[:, None]).astype(np.int32)
    dm = (np.arange(Ld)[None] < dl[:, None]).astype(np.int32)
    if Ld > 4:
        holes = r.random((N, Ld)) < 0.15
        dm[holes] = 0
        dm[np.arange(N), 0] = 1
    if Lq > 4:
        qm[r.random((B, Lq)) < 0.15] = 0
        qm[np.arange(B), 0] = 1
    if N > 1:
        dm[N - 1] = 0
    if B > 1:
        qm[B - 1] = 0
    # padding holds large values, as an encoder's padded positions may: counting a masked token shows in the scores
    d[dm == 0] *= 4.0
    q[qm == 0] *= 4.0
    return q, d, qm, dm


def gap_floor(q, d):
    """Twice the f32 accumulation error bound of one dot product, E 2^-24 max|q_i| max|d_j|: where the best and the
    second-best document token differ by more, the device's argmax must equal the reference's."""
    q, d = np.asarray(q, np.float64), np.asarray(d, np.float64)
    E = q.shape[-1]
    return 2.0 * E * 2.0 ** -24 * float(np.sqrt((q * q).sum(-1)).max() * np.sqrt((d * d).sum(-1)).max())
