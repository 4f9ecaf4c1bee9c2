"""The tolerances of test_crf_gpu.py can see the bugs they are there to catch, and can be met (float64 oracle and float32
NumPy restatements only: no GPU, no library).

Each perturbation below is applied to the float64 reference alone, on every case of tests/crf_cases.py it applies to
(every shape, with and without sample weights, with and without accumulate), and must move at least one output by 5x the
tolerance the GPU test applies to that output:
  a length off by one; transitions transposed; an out-of-range tag dropped instead of clamped; sample weights ignored;
  the mean over B replaced by a mean over the non-empty sequences; accumulate ignoring the prior dtrans; the gold
  transition into position L counted.
The references themselves are held too: the scaled-domain restatement without the rescue (the arithmetic crf.hip had) meets
the bounds of the BIO margin cases up to M = 60 and misses them 5x over from M = 95 on and at scale 100, so the GPU test
sees that underflow; the arithmetic crf.hip has now (rescue=True) meets every one of them; every float32 restatement stays within half of the bounds derived from
it, and within half of the suite's bounds on the table's own shapes."""
import numpy as np
import pytest

from oracle import losses as ol
from tests import crf_cases as cc
from tests import crf_ref as cr

MARGIN = 5.0


# ------------------------------------------------------------------------------------------------- perturbations
def ref64(inp, weights=None, prior=None, *, lengths=None, trans=None, drop=(), mean_nonempty=False, into_L=False):
    """The reference from oracle.losses.crf_log_likelihood sequence by sequence, with the hooks of the perturbations."""
    B, S, C = inp.shape
    L = inp.L if lengths is None else lengths
    T = (inp.trans if trans is None else trans).astype(np.float64)
    x, t = inp.pot.astype(np.float64), inp.t
    w = np.ones(B) if weights is None else weights.astype(np.float64)
    D = max(1, int((L > 0).sum())) if mean_nonempty else B
    loss, dpot = 0.0, np.zeros((B, S, C))
    dT = np.zeros((C, C)) if prior is None else prior.astype(np.float64).copy()
    for b in range(B):
        ll, dx, dTb = ol.crf_log_likelihood(x[b:b + 1], t[b:b + 1], L[b:b + 1], T)
        ll = ll[0]
        Lb = int(L[b])
        for bb, s, _ in drop:                   # this position's gold emission and both gold transitions vanish
            if bb == b and s < Lb:
                ll -= x[b, s, t[b, s]]
                dx[0, s, t[b, s]] -= 1.0
                if s > 0:
                    ll -= T[t[b, s - 1], t[b, s]]
                    dTb[t[b, s - 1], t[b, s]] -= 1.0
                if s + 1 < Lb:
                    ll -= T[t[b, s], t[b, s + 1]]
                    dTb[t[b, s], t[b, s + 1]] -= 1.0
        if into_L and 0 < Lb < S:
            ll += T[t[b, Lb - 1], t[b, Lb]]
            dTb[t[b, Lb - 1], t[b, Lb]] += 1.0
        loss += -ll * w[b] / D
        dpot[b] = -dx[0] * w[b] / D
        dT += -dTb * w[b] / D
    return {"loss": loss, "dpot": dpot, "dtrans": dT}


def violation(pert, base, tol):
    e = cc.errors(pert, base)
    return max(e[k] / tol[k] for k in e)


def perturbations(inp, weights, prior):
    """(what, perturbed reference) for every perturbation that applies to this case."""
    B, S, C = inp.shape
    kw = dict(weights=weights, prior=prior)
    if prior is not None:
        yield "accumulate ignoring the prior dtrans", ref64(inp, weights, None)
    if C == 1:
        return                                  # one tag: loss and gradients are zero whatever the inputs
    if weights is not None:
        yield "sample weights ignored", ref64(inp, None, prior)
    L = inp.L if weights is None else np.where(weights > 0, inp.L, 0)       # a weight-0 sequence cannot show the rest
    if (L > 0).any():
        yield "a length off by one", ref64(inp, lengths=np.maximum(inp.L - 1, 0), **kw)
    if (L > 1).any():
        yield "transitions transposed", ref64(inp, trans=inp.trans.T, **kw)
    if ((L > 0) & (L < S)).any():
        yield "the gold transition into position L counted", ref64(inp, into_L=True, **kw)
    if any(L[b] > 0 for b, _, _ in inp.oor):
        yield "an out-of-range tag dropped", ref64(inp, drop=inp.oor, **kw)
    if (inp.L == 0).any() and (L > 0).any():
        yield "mean over the non-empty sequences", ref64(inp, mean_nonempty=True, **kw)


@pytest.mark.parametrize("B,S,C", cc.SHAPES, ids=lambda v: str(v))
def test_crf_tolerances_see_the_perturbations(B, S, C):
    inp = cc.nll_inputs(B, S, C)
    seen = set()
    for weights in (None, inp.weights):
        for prior in (None, inp.prior):
            base = cc.reference(inp, weights, prior)
            mine = ref64(inp, weights, prior)
            assert violation(mine, base, cc.tolerances("f32")) < 1e-6       # the hooks off: crf_nll_fwd itself
            for what, pert in perturbations(inp, weights, prior):
                seen.add(what)
                for dtype in cc.DTYPES:
                    v = violation(pert, base, cc.tolerances(dtype))
                    assert v >= MARGIN, f"{B}x{S}x{C} w={weights is not None} acc={prior is not None} {dtype}: {what} " \
                                        f"moves the reference by only {v:.2f}x the tolerance"
    assert "accumulate ignoring the prior dtrans" in seen
    if C > 1 and B >= 7:
        assert len(seen) == 7, seen


# ------------------------------------------------------------------------------------------------- the table
def test_crf_table_covers_both_paths_and_their_edges():
    small, wg = [s for s in cc.SHAPES if s[2] <= cc.CRF_MAXC], [s for s in cc.SHAPES if s[2] > cc.CRF_MAXC]
    assert tuple(small) == cc.SMALL_SHAPES and tuple(wg) == cc.WG_SHAPES
    assert {1, 16} <= {C for _, _, C in small} and {17, 128} <= {C for _, _, C in wg}
    assert {32, 33, 64, 65} <= {C for _, _, C in wg}
    assert [cc.bucket(C) for C in (16, 17, 32, 33, 64, 65, 128)] == [0, 32, 32, 64, 64, 128, 128]
    assert any(B > 64 and B % 64 for B, _, _ in small)                       # a second 64-thread block, partly idle
    assert any(S > cc.workgroup(C) and cc.bucket(C) <= 64 for _, S, C in wg)
    assert any(S > cc.workgroup(C) and cc.bucket(C) == 128 for _, S, C in wg)
    for path in (small, wg):
        assert set().union(*(cc.length_classes(B, cc.phase(B, S, C)) for B, S, C in path)) == set(cc.LENGTH_CLASSES)
    assert set(cc.DTYPES) == {"f32", "bf16"}
    assert {2 + 2 * n for n in cc.BIO_TYPES} == {16, 26, 64, 128}
    assert all(C >= 4 for _, _, C in cc.VITERBI_SHAPES) and len(cc.VITERBI_SHAPES) == len(cc.SHAPES) - 2
    assert set(cc.LONG_TOL) == set(cc.LONG_SHAPES) and set(cc.BIO_TOL) == set(cc.BIO_CASES)


@pytest.mark.parametrize("B,S,C", cc.SHAPES, ids=lambda v: str(v))
def test_crf_inputs_are_what_the_table_says(B, S, C):
    inp = cc.nll_inputs(B, S, C)
    value = dict(zip(cc.LENGTH_CLASSES, (S, 0, 1, 2, S - 1, S + 5, -3)))
    assert {value[k] for k in cc.length_classes(B, cc.phase(B, S, C))} == set(inp.lengths[:7]) and inp.lengths.dtype == np.int32
    L = inp.L
    assert L.min() >= 0 and L.max() <= S and L[0] == S
    for b in range(B):
        assert (inp.tags[b, L[b]:] == cc.PAST_L_TAG).all()
        inside = inp.tags[b, :L[b]]
        bad = [(bb, s, v) for bb, s, v in inp.oor if bb == b]
        assert ((inside < 0) | (inside >= C)).sum() == len(bad)
        assert all(inp.tags[bb, s] == v and s < L[bb] for bb, s, v in bad)
    assert [v for _, _, v in inp.oor] == ([-1, C + 3] if B * S > 1 else [-1])
    assert (inp.weights == 0).sum() == 1 and L[inp.weights == 0][0] > 0 and inp.weights.dtype == np.float32
    assert inp.t.min() >= 0 and inp.t.max() <= C - 1


# ------------------------------------------------------------------------------------------------- the references
def _restated(fn, inp, weights=None, prior=None, lengths="own", **kw):
    loss, dpot, dT = fn(inp.pot, inp.tags, None if lengths is None else inp.lengths, inp.trans, weights, prior, **kw)
    return {"loss": loss, "dpot": dpot, "dtrans": dT}


@pytest.mark.parametrize("B,S,C", cc.SHAPES, ids=lambda v: str(v))
def test_f32_arithmetic_meets_half_the_suite_bounds_on_the_table(B, S, C):
    """Both formulations in float32 on every call the GPU test makes at this shape: the bounds can be met."""
    inp = cc.nll_inputs(B, S, C)
    tol = cc.tolerances("f32")
    for weights, prior, lengths in ((None, None, "own"), (inp.weights, inp.prior, "own"), (inp.weights, None, None)):
        ref = cc.reference(inp, weights, prior, lengths=lengths)
        for fn, kw in ((cr.nll_log, {}), (cr.nll_scaled, {}), (cr.nll_scaled, {"rescue": True})):
            v = violation(_restated(fn, inp, weights, prior, lengths, **kw), ref, tol)
            assert v <= 0.5, (fn.__name__, kw, weights is not None, lengths, v)


@pytest.mark.parametrize("B,S,C", cc.LONG_SHAPES, ids=lambda v: str(v))
def test_long_bounds_come_from_the_restatements(B, S, C):
    inp = cc.long_inputs(B, S, C)
    ref = cc.reference(inp)
    tol = cc.LONG_TOL[(B, S, C)]
    assert tol == cc.derived_tol(*cc.LONG_MEASURED[(B, S, C)].values())
    for name, fn in (("log", cr.nll_log), ("scaled", cr.nll_scaled)):
        err = cc.errors(_restated(fn, inp), ref)
        for k in err:
            assert err[k] <= tol[k] / 2, (name, k, err[k], tol[k])
    # what crf.hip computes now (crf_ref.nll_split; no rescue is taken on these inputs) meets them too
    err = cc.errors(_restated(cr.nll_scaled, inp, rescue=True), ref)
    for k in err:
        assert err[k] <= tol[k] / 2, ("rescued", k, err[k], tol[k])


def _bio_err(fn, inp, **kw):
    loss, dpot, dT = fn(inp.pot, inp.tags, inp.lengths, inp.trans, **kw)
    assert inp.mask is not None
    return cc.errors(cc.bio_got(inp, loss, dpot, dT), cc.bio_reference(inp))


@pytest.mark.parametrize("kind,n_types,v", cc.BIO_CASES, ids=lambda v: str(v))
def test_bio_bounds_come_from_the_log_domain_and_see_the_floor(kind, n_types, v):
    inp = cc.bio_inputs(kind, n_types, v)
    C = inp.shape[2]
    tol = cc.BIO_TOL[(kind, n_types, v)]
    # gold obeys the mask; the margin construction is the one the bound is about
    assert all(inp.mask[a, b] for row in inp.tags for a, b in zip(row[:-1], row[1:]))
    if kind == "margin":
        assert (inp.tags[:, 4] == cc.B0).all() and (inp.tags[:, 5] == cc.I0).all() and (np.delete(inp.tags, (4, 5), 1) == cc.O).all()
        assert inp.mask[cc.O, cc.I0] == 0 and inp.trans[cc.O, cc.I0] == -10000
    err = _bio_err(cr.nll_log, inp)
    for k in err:
        assert err[k] <= tol[k] / 2, ("log", k, err[k], tol[k])
    if C <= cc.CRF_MAXC:
        return                                  # served by the log-domain kernels
    worst = max(e / tol[k] for k, e in _bio_err(cr.nll_scaled, inp).items())
    if kind == "margin" and v <= 60:
        assert worst <= 0.5, worst
    if (kind == "margin" and v >= 95) or (kind == "scale" and v == 100):
        assert worst >= MARGIN, f"the floored arithmetic misses the bound by only {worst:.2f}x"


# What crf.hip computes now (crf_ref.nll_split: rescues, shared part of alpha and beta in float64) against the log-domain
# bounds, each case's own.
@pytest.mark.parametrize("kind,n_types,v", [c for c in cc.BIO_CASES if 2 + 2 * c[1] > cc.CRF_MAXC], ids=lambda v: str(v))
def test_rescued_restatement_meets_the_bio_bounds(kind, n_types, v):
    inp = cc.bio_inputs(kind, n_types, v)
    tol = cc.BIO_TOL[(kind, n_types, v)]
    err = _bio_err(cr.nll_scaled, inp, rescue=True)
    for k in err:
        assert err[k] <= tol[k], (k, err[k], tol[k])


def test_viterbi_grid_is_exact_in_f32():
    for B, S, C in cc.VITERBI_SHAPES:
        pot, lengths, trans = cc.viterbi_inputs(B, S, C)
        assert np.array_equal(pot * 16, np.round(pot * 16)) and np.abs(pot).max() <= 4
        assert np.array_equal(trans * 16, np.round(trans * 16)) and np.abs(trans).max() <= 0.5
        if C >= 6:
            assert np.array_equal(pot[:, :, C - 3:], pot[:, :, :3]) and np.array_equal(trans[C - 3:, C - 3:], trans[:3, :3])
        assert lengths[0] == S and (B < 7 or {0, 1, 2, S - 1, S + 5, -3} <= set(lengths))
    for n in cc.BIO_TYPES:
        mask = cc.bio_mask(n)
        pot, _, trans = cc.viterbi_inputs(cc.VITERBI_BIO_B, cc.VITERBI_BIO_S, mask.shape[0], mask)
        assert set(np.unique(trans[mask == 0])) == {-10000.0}
        # even an all-masked path stays below 2^24 sixteenths: every f32 sum is exact
        assert cc.VITERBI_BIO_S * (10000 + 4.5) * 16 < 2 ** 24
