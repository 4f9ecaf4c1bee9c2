"""float32 NumPy restatements of the two CRF formulations (host only; no GPU, no library).

  nll_log     the log-domain recurrences of crf_nll_kernel (polus_amd/csrc/loss.hip, C <= 16): alpha and beta by
              max + log(sum(exp(. - max))), marginals exp(alpha + beta - logZ), pair marginals
              exp(alpha_prev[k] + T[k][j] + x[j] + beta[j] - logZ).
  nll_scaled  the scaled-domain recurrences of crf_nll_wg_kernel (polus_amd/csrc/crf.hip, 17 <= C <= 128) without its
              log-domain rescue: E = exp(T - column max), a = exp(alpha - max(alpha)), the GEMV sums floored at FLT_MIN
              before the log, marginals a * exp(beta + m - logZ), pair marginals E[k][j] * sum_s a_prev[k] *
              exp(m_prev + n - logZ) * q[j].  This is the arithmetic the kernel had before the rescue, kept so that
              test_crf_cases_cpu.py can show that the bounds of the BIO margin cases see the underflow it had.
              rescue=True gives nll_split instead.
  nll_split   what crf.hip computes now: see its docstring.

Every intermediate is float32 (inputs are cast on entry; numpy keeps float32 through +, *, max).  exp and log are taken
in float64 and rounded to float32, so that the figures tabulated in tests/crf_cases.py do not depend on which SIMD
implementation of the float32 functions numpy picks on the machine at hand.  The order of the additions inside a sum is
numpy's, not the kernels': the derived bounds of tests/crf_cases.py double the restatements' error for that.  Both return
(loss, dpot [B,S,C], dtrans [C,C]) as float32 for clamped lengths and tags, sample weights (or None) and a prior dtrans
(accumulate) or None."""
import numpy as np

F = np.float32
FLT_MIN = F(np.finfo(np.float32).tiny)
RESCUE_SUM, RESCUE_EXP = F(1e-25), F(40)         # CRF_RESCUE_SUM, CRF_RESCUE_EXP of crf.hip


def _exp(v):
    return np.exp(np.asarray(v, np.float64)).astype(F)


def _log(v):
    return np.log(np.asarray(v, np.float64)).astype(F)


def _clamp(tags, lengths, S, C):
    L = np.clip(np.asarray(lengths, np.int64), 0, S)
    return np.clip(np.asarray(tags, np.int64), 0, C - 1), L


def _lse(v, axis):
    mx = v.max(axis, keepdims=True)
    return (mx + _log(_exp(v - mx).sum(axis, keepdims=True, dtype=F))).squeeze(axis)


def _score(x, T, t, L):
    sc = F(0)
    for s in range(L):
        sc = sc + x[s, t[s]]
        if s + 1 < L:
            sc = sc + T[t[s], t[s + 1]]
    return sc


def _finish(nll_b, dT_b, B, prior):
    s = F(0)
    for v in nll_b:
        s = s + v
    dT = np.zeros_like(dT_b[0])
    for d in dT_b:
        dT = dT + d
    if prior is not None:
        dT = np.asarray(prior, F) + dT
    return F(s / F(B)), dT


def nll_log(pot, tags, lengths, trans, sample_w=None, prior=None):
    x_all, T = np.asarray(pot, F), np.asarray(trans, F)
    B, S, C = x_all.shape
    tags, lengths = _clamp(tags, lengths if lengths is not None else np.full(B, S), S, C)
    dpot = np.zeros((B, S, C), F)
    nll_b, dT_b = [], []
    with np.errstate(all="ignore"):
        for b in range(B):
            x, t, L = x_all[b], tags[b], int(lengths[b])
            wsw = F(1) if sample_w is None else F(sample_w[b])
            w = F(wsw / F(B))
            dT = np.zeros((C, C), F)
            if L == 0:
                nll_b.append(F(0)); dT_b.append(dT)
                continue
            al = np.zeros((L, C), F)
            al[0] = x[0]
            for s in range(1, L):
                al[s] = _lse(al[s - 1][:, None] + T, 0) + x[s]
            logz = _lse(al[L - 1], 0)
            nll_b.append(F(-(_score(x, T, t, L) - logz) * wsw))
            beta = np.zeros(C, F)
            for s in range(L - 1, -1, -1):
                marg = _exp(al[s] + beta - logz)
                marg[t[s]] -= F(1)
                dpot[b, s] = marg * w
                if s > 0:
                    tmp = T + (x[s] + beta)[None, :]
                    pair = _exp(al[s - 1][:, None] + tmp - logz)
                    pair[t[s - 1], t[s]] -= F(1)
                    dT = dT + pair * w
                    beta = _lse(tmp, 1)
            dT_b.append(dT)
    loss, dT = _finish(nll_b, dT_b, B, prior)
    return loss, dpot, dT


def nll_scaled(pot, tags, lengths, trans, sample_w=None, prior=None, rescue=False):
    if rescue:
        return nll_split(pot, tags, lengths, trans, sample_w, prior)
    x_all, T = np.asarray(pot, F), np.asarray(trans, F)
    B, S, C = x_all.shape
    tags, lengths = _clamp(tags, lengths if lengths is not None else np.full(B, S), S, C)
    dpot = np.zeros((B, S, C), F)
    nll_b, dT_b = [], []
    with np.errstate(all="ignore"):
        cmax = T.max(0)
        E = _exp(T - cmax[None, :])
        for b in range(B):
            x, t, L = x_all[b], tags[b], int(lengths[b])
            wsw = F(1) if sample_w is None else F(sample_w[b])
            w = F(wsw / F(B))
            if L == 0:
                nll_b.append(F(0)); dT_b.append(np.zeros((C, C), F))
                continue
            a, m = np.zeros((L, C), F), np.zeros(L, F)
            alpha = x[0].copy()
            for s in range(L):
                m[s] = alpha.max()
                a[s] = _exp(alpha - m[s])
                if s + 1 == L:
                    break
                sm = (a[s][:, None] * E).sum(0, dtype=F)
                alpha = x[s + 1] + cmax + m[s] + _log(np.maximum(sm, FLT_MIN))
            logz = m[L - 1] + _log(a[L - 1].sum(dtype=F))
            nll_b.append(F(-(_score(x, T, t, L) - logz) * wsw))
            acc = np.zeros((C, C), F)
            beta = np.zeros(C, F)
            for s in range(L - 1, -1, -1):
                marg = a[s] * _exp(beta + (m[s] - logz))
                marg[t[s]] -= F(1)
                dpot[b, s] = marg * w
                if s == 0:
                    break
                v = x[s] + beta + cmax
                n = v.max()
                q = _exp(v - n)
                ck = a[s - 1] * _exp(m[s - 1] + n - logz)          # 0 * inf = NaN where a_prev has underflowed
                acc = acc + ck[:, None] * q[None, :]
                beta = n + _log(np.maximum((E * q[None, :]).sum(1, dtype=F), FLT_MIN))
            dT = E * acc
            for s in range(1, L):
                dT[t[s - 1], t[s]] -= F(1)
            dT_b.append(dT * w)
    loss, dT = _finish(nll_b, dT_b, B, prior)
    return loss, dpot, dT


def nll_split(pot, tags, lengths, trans, sample_w=None, prior=None):
    """What crf_nll_wg_kernel computes now.  alpha[j] = M + d[j] and beta[k] = N + e[k]: the uniform parts M, N (and logZ)
    are float64 scalars, the per-tag parts float32 of small magnitude, and the two are never added in float32, so the
    roundings no longer grow with |alpha|.  Per step  dm = max(d), a = exp(d - dm), M' = M + dm,
    d'[j] = (x[j] + cmax_j) + log(sum_k a[k] E[k][j]);  v = (x + e) + cmax, vm = max(v), q = exp(v - vm), N' = N + vm,
    e'[k] = log(sum_j E[k][j] q[j]).  A sum under RESCUE_SUM is recomputed in the log domain, d'[j] = x[j] + (lse_k(d[k] +
    T[k][j]) - dm) resp. e'[k] = lse_j(T[k][j] + x[j] + e[j]) - vm; a marginal a * exp(e + c), c = M + dm + N - logZ, is
    exp(log a + (e + c)) where e + c > RESCUE_EXP; a step whose g = c_prev + vm > RESCUE_EXP adds its pair marginals
    exp(log a_prev[k] + T[k][j] + x[j] + e[j] + c_prev) directly."""
    x_all, T = np.asarray(pot, F), np.asarray(trans, F)
    B, S, C = x_all.shape
    tags, lengths = _clamp(tags, lengths if lengths is not None else np.full(B, S), S, C)
    dpot = np.zeros((B, S, C), F)
    nll_b, dT_b = [], []
    D = np.float64
    with np.errstate(all="ignore"):
        cmax = T.max(0)
        E = _exp(T - cmax[None, :])
        for b in range(B):
            x, t, L = x_all[b], tags[b], int(lengths[b])
            wsw = F(1) if sample_w is None else F(sample_w[b])
            w = F(wsw / F(B))
            if L == 0:
                nll_b.append(F(0)); dT_b.append(np.zeros((C, C), F))
                continue
            a, la, dm = np.zeros((L, C), F), np.zeros((L, C), F), np.zeros(L, F)
            Mm = np.zeros(L, D)                                 # M + dm: the step's largest alpha
            d, M = x[0].copy(), D(0)
            for s in range(L):
                dm[s] = d.max()
                la[s] = d - dm[s]
                a[s] = _exp(la[s])
                Mm[s] = M + D(dm[s])
                if s + 1 == L:
                    break
                sm = (a[s][:, None] * E).sum(0, dtype=F)
                dn = (x[s + 1] + cmax) + _log(np.maximum(sm, FLT_MIN))
                d = np.where(sm >= RESCUE_SUM, dn, x[s + 1] + (_lse(d[:, None] + T, 0) - dm[s]))
                M = Mm[s]
            logz = Mm[L - 1] + D(_log(a[L - 1].sum(dtype=F)))
            nll_b.append(F(-(_score(x, T, t, L) - F(logz)) * wsw))
            acc, direct = np.zeros((C, C), F), np.zeros((C, C), F)
            e, N = np.zeros(C, F), D(0)
            for s in range(L - 1, -1, -1):
                c = F(Mm[s] + N - logz)
                ec = e + c
                a_s = np.where(a[s] >= FLT_MIN, a[s], F(0))
                marg = np.where(ec > RESCUE_EXP, _exp(la[s] + ec), a_s * _exp(ec))
                marg[t[s]] -= F(1)
                dpot[b, s] = marg * w
                if s == 0:
                    break
                u = x[s] + e
                v = u + cmax
                vm = v.max()
                q = _exp(v - vm)
                cp = F(Mm[s - 1] + N - logz)
                g = F(Mm[s - 1] + (N + D(vm)) - logz)
                if g > RESCUE_EXP:
                    direct = direct + _exp((la[s - 1][:, None] + T + u[None, :]) + cp)
                else:
                    a_p = np.where(a[s - 1] >= FLT_MIN, a[s - 1], F(0))
                    acc = acc + (a_p * _exp(g))[:, None] * q[None, :]
                sm = (E * q[None, :]).sum(1, dtype=F)
                e = np.where(sm >= RESCUE_SUM, _log(np.maximum(sm, FLT_MIN)), _lse(T + u[None, :], 1) - vm)
                N = N + D(vm)
            dT = E * acc + direct
            for s in range(1, L):
                dT[t[s - 1], t[s]] -= F(1)
            dT_b.append(dT * w)
    loss, dT = _finish(nll_b, dT_b, B, prior)
    return loss, dpot, dT
