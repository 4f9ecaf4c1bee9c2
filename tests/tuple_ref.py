"""float64 NumPy references of tuple scoring and the distillation losses (polus_amd/csrc/tuples.hip), test
infrastructure only: query b is scored against its own n documents, document (b, j) at row j*B + b (layout 0) or
b*n + j (layout 1).  Also plain float32 restatements of the two losses and the dot, the measure of what f32 arithmetic
alone costs against float64.

A column whose teacher score is -inf is absent: left out of every sum, zero gradient, its student value unused."""
import numpy as np

from tests import maxsim_ref


def doc_rows(B, n, layout):
    """rows[b, j] = the row of document (b, j)."""
    b, j = np.arange(B)[:, None], np.arange(n)[None, :]
    return (j * B + b) if layout == 0 else (b * n + j)


# ---------------------------------------------------------------------------------------------- MaxSim tuples
def maxsim_tuples_fwd(q, d, qmask, dmask, layout):
    """(score [B, n], argmax int32 [B, n, Lq]) from maxsim_ref.maxsim_fwd of every pair on its own."""
    B, Lq, _ = q.shape
    n = d.shape[0] // B
    rows = doc_rows(B, n, layout)
    score = np.zeros((B, n))
    am = np.zeros((B, n, Lq), np.int32)
    for b in range(B):
        for j in range(n):
            r = rows[b, j]
            s, a = maxsim_ref.maxsim_fwd(q[b:b + 1], d[r:r + 1], None if qmask is None else qmask[b:b + 1],
                                         None if dmask is None else dmask[r:r + 1])
            score[b, j], am[b, j] = s[0, 0], a[0, 0]
    return score, am


def maxsim_tuples_bwd(q, d, dscore, argmax, layout):
    """(dq [B, Lq, E], dd [B n, Ld, E]) of sum(dscore * score) given the argmax [B, n, Lq]."""
    q, d, dscore = (np.asarray(a, np.float64) for a in (q, d, dscore))
    B = q.shape[0]
    n = d.shape[0] // B
    rows = doc_rows(B, n, layout)
    dq, dd = np.zeros_like(q), np.zeros_like(d)
    for b in range(B):
        for j in range(n):
            a = argmax[b, j]
            hit = a >= 0
            if hit.any():
                dq[b, hit] += dscore[b, j] * d[rows[b, j], a[hit]]
                np.add.at(dd[rows[b, j]], a[hit], dscore[b, j] * q[b, hit])
    return dq, dd


# ---------------------------------------------------------------------------------------------- dot tuples
def dot_tuples_fwd(q, d, layout, dtype=np.float64, skip=None):
    """score [B, n]; `skip` = (b, j, w): that one term is left out (the mistake of tests/test_tuples_cpu.py)."""
    q, d = np.asarray(q, dtype), np.asarray(d, dtype)
    B = q.shape[0]
    n = d.shape[0] // B
    prod = q[:, None, :] * d[doc_rows(B, n, layout)]
    if skip is not None:
        prod[skip] = 0
    return prod.sum(-1, dtype=dtype)


def dot_tuples_bwd(q, d, dscore, layout, dtype=np.float64):
    q, d, dscore = (np.asarray(a, dtype) for a in (q, d, dscore))
    B = q.shape[0]
    n = d.shape[0] // B
    rows = doc_rows(B, n, layout)
    dq = (dscore[:, :, None] * d[rows]).sum(1, dtype=dtype)
    dd = np.zeros_like(d)
    dd[rows] = dscore[:, :, None] * q[:, None, :]
    return dq, dd


# ---------------------------------------------------------------------------------------------- losses
def _present(t):
    return ~np.isneginf(np.asarray(t, np.float64))


def _log_softmax(x, on, dtype):
    """log-softmax over the columns where `on`, -inf elsewhere; rows without a column give -inf throughout."""
    x = np.where(on, np.asarray(x, dtype), dtype(-np.inf))
    mx = np.where(on.any(1, keepdims=True), x.max(1, keepdims=True), dtype(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.exp(x - mx, dtype=dtype).sum(1, keepdims=True, dtype=dtype)
        return ((x - mx) - np.log(np.where(z > 0, z, dtype(1)), dtype=dtype)).astype(dtype)


def _count(s, t, on, cell):
    """Mistake: the absent column `cell` = (row, col) is counted, with the values found there (a teacher score of
    -inf, and whatever the student holds: the cases of tests/tuple_cases.py put NaN there)."""
    on = on.copy()
    assert not on[cell]
    on[cell] = True
    return s, t, on


def distill_kl(student, teacher, dtype=np.float64, count_absent=None, drop_mean=False, swap=False):
    """(loss, dstudent) of the mean over the rows of KL(softmax(teacher) || softmax(student)) over the present columns.
    The keyword switches are the mistakes of tests/test_tuples_cpu.py: one absent column counted, the 1 / rows dropped,
    teacher and student swapped in the gradient."""
    dtype = np.dtype(dtype).type
    s, t = np.asarray(student, dtype), np.asarray(teacher, dtype)
    on = _present(teacher)
    if count_absent is not None:
        s, t, on = _count(s, t, on, count_absent)
    s = np.where(on, s, dtype(0))
    rows = dtype(1 if drop_mean else s.shape[0])
    lp, ls = _log_softmax(t, on, dtype), _log_softmax(s, on, dtype)
    p = np.where(on, np.exp(lp, dtype=dtype), dtype(0))
    with np.errstate(invalid="ignore"):
        loss = np.where(on, p * (lp - ls), dtype(0)).sum(dtype=dtype) / rows
    sm = np.where(on, np.exp(ls, dtype=dtype), dtype(0))
    g = ((p - sm) if swap else (sm - p)) / rows
    return dtype(loss), g.astype(dtype)


def margin_mse(student, teacher, dtype=np.float64, count_absent=None, drop_mean=False, positive=0):
    """(loss, dstudent) of the mean over the present negatives j != positive of every row whose positive column is
    present of ((s_pos - s_j) - (t_pos - t_j))^2; the positive is column 0.  Switches (tests/test_tuples_cpu.py): one
    absent negative counted, the 1 / M dropped, another column taken as the positive."""
    dtype = np.dtype(dtype).type
    s, t = np.asarray(student, dtype), np.asarray(teacher, dtype)
    on = _present(teacher)
    if count_absent is not None:
        s, t, on = _count(s, t, on, count_absent)
    neg = on & on[:, positive:positive + 1]
    neg[:, positive] = False
    used = neg | ((np.arange(t.shape[1]) == positive)[None, :] & on)
    s, t = np.where(used, s, dtype(0)), np.where(used, t, dtype(0))
    M = dtype(1 if drop_mean else max(int(neg.sum()), 1))
    e = np.where(neg, (s[:, positive:positive + 1] - s) - (t[:, positive:positive + 1] - t), dtype(0)).astype(dtype)
    loss = (e * e).sum(dtype=dtype) / M
    g = -dtype(2) * e / M
    g[:, positive] = dtype(2) * e.sum(1, dtype=dtype) / M
    return dtype(loss), g.astype(dtype)


