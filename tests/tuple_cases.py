"""Cases and tolerances of the tuple-scoring and distillation tests (tests/test_tuples_cpu.py, tests/test_tuples_gpu.py).

MaxSim tuples are held to tests/maxsim_cases.TOL unchanged: their bits are those of the all-pairs kernels."""
import numpy as np

from tests.maxsim_cases import make_case

# (B, n, Lq, Ld, E): B queries with n documents each
SHAPES = [(1, 1, 1, 1, 32), (3, 2, 5, 17, 32), (4, 3, 31, 65, 64),
          (5, 4, 33, 180, 128),        # three query tiles, a ragged last document tile
          (2, 2, 64, 512, 256),        # the largest of every limit: the query does not fit one wave's registers
          (2, 70, 8, 24, 64)]          # more documents per query than one workgroup's four waves take
MASKS = ["none", "ragged"]
LAYOUTS = [0, 1]

LOSS_SHAPES = [(1, 2), (3, 3), (7, 64), (5, 65), (2, 1024)]      # rows x n
DOT_W = [1, 33, 128, 30522]                                     # with (B, n) = DOT_BN
DOT_BN = (2, 2)

# relative to max|reference| over the tensor (tests/util.relerr); set at 2-3x the worst error measured on one MI355X
# over the cases above:
#   dot f32    score 6.6e-7 (W = 30522: a lane's fmaf chain is 480 terms long), dq 7.8e-8, dd 5.0e-8
#   dot bf16   score 0 (products of bf16 values of this magnitude and their sums fit f32 exactly; the arithmetic is
#              the f32 engine's, so its bound is kept), dq 3.5e-3, dd 2.8e-3 (rounded to bf16 once, half an ulp 2.0e-3)
#   KL         loss 4.3e-5 (the 1 x 2 case: a loss of 2.3e-3 left after cancellation among scores of order 30),
#              gradient 7.8e-6 (same case)
#   MarginMSE  loss 8.7e-7, gradient 4.8e-7
# The float32 NumPy restatement of tests/tuple_ref.py has to pass them as well (tests/test_tuples_cpu.py); its worst
# errors are 2.4e-7 / 9.3e-8 (dot score / gradients), 4.2e-5 / 7.8e-6 (KL) and 8.7e-7 / 4.8e-7 (MarginMSE): the two
# losses lose in f32 what the device loses.
TOL = {
    "dot_f32": dict(score=1.6e-6, grad=2.2e-7),
    "dot_bf16": dict(score=1.6e-6, grad=8e-3),
    "kl": dict(loss=1.1e-4, grad=2e-5),
    "mse": dict(loss=2.2e-6, grad=1.2e-6),
}


def tuple_case(shape, masks):
    """maxsim_cases.make_case over the B n documents of a tuple shape: q [B, Lq, E], d [B n, Ld, E], masks or None."""
    B, n, Lq, Ld, E = shape
    return make_case((B, n - 1, Lq, Ld, E), masks)


def loss_case(rows, n, kind, seed=0):
    """(student, teacher) f32 [rows, n].  Student scores at MaxSim scale (|s| up to about 32), the last row at +-80 so
    that a softmax without its maximum subtracted overflows; teacher scores likewise.  Absent columns (teacher -inf)
    are scattered, their student value is NaN (it must not be used); one row has every column absent (rows >= 3);
    for kind "mse" one more row has column 0 absent (rows >= 5)."""
    r = np.random.Generator(np.random.PCG64(500 + 13 * rows + n + seed))
    s = (r.uniform(-32, 32, size=(rows, n))).astype(np.float32)
    t = (s + r.standard_normal((rows, n)) * 3.0).astype(np.float32)
    s[rows - 1] = np.where(r.random(n) < 0.5, 80.0, -80.0).astype(np.float32) + r.standard_normal(n).astype(np.float32)
    t[rows - 1] = (s[rows - 1] * 0.9).astype(np.float32)
    if n > 2:
        absent = r.random((rows, n)) < 0.15
        absent[:, 0] = False
        absent[np.arange(rows), 1 + r.integers(0, n - 1, size=rows)] = False      # every row keeps a negative
        t[absent] = -np.inf
    if rows >= 3:
        t[1] = -np.inf
    if kind == "mse" and rows >= 5:
        t[2, 0] = -np.inf
    s[np.isneginf(t)] = np.nan
    return s, t


def dot_case(W, seed=0):
    """q [B, W], d [B n, W] float32 and dscore [B, n].  Magnitudes in [0.5, 1.5) with random signs: no term of a dot
    product is negligible, so a dropped one shows in the score."""
    B, n = DOT_BN
    r = np.random.Generator(np.random.PCG64(900 + W + seed))
    val = lambda *shape: (r.uniform(0.5, 1.5, size=shape) * r.choice([-1.0, 1.0], size=shape)).astype(np.float32)
    return val(B, W), val(B * n, W), r.standard_normal((B, n)).astype(np.float32)
