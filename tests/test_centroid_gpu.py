"""The centroid kernels on the device against the NumPy / float64 reference of tests/centroid_ref.py:
polus_centroid_scores (bit for bit on integer tables over every lane mapping and both routes, the route boundary,
independence of the launch, an f32 summation bound on N(0, 1) tables), polus_centroid_codes (exact, ties, NaN, masks,
strides) and polus_centroid_update (exact counts, a derived bound on the centroids, kept rows, equal bits twice)."""
import numpy as np
import pytest
import torch

from tests import centroid_ref as cr
from tests.centroid_cases import (CODE_SHAPES, GLOBAL_SHAPES, LDS_BYTES, NONE, SCORE_SHAPES, UPDATE_SHAPES, code_case,
                                  score_case, update_case)
from tests.util import rounded

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
GUARD = -7.25


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _codes_dev(codes):
    return torch.as_tensor(np.ascontiguousarray(codes).view(np.int16)).cuda()


def _scores(table, qmask, codes, B, Lq):
    """One polus_centroid_scores launch: the table keeps its guard columns (ldt > B*Lq), the scores land in a [B, N + 5]
    buffer (lds > N) whose last columns must stay as they were."""
    from polus_amd import ops
    N = codes.shape[0]
    t = torch.as_tensor(table).cuda()
    buf = torch.full((B, N + 5), GUARD, dtype=torch.float32, device="cuda")
    ops.centroid_scores(t, None if qmask is None else torch.as_tensor(qmask).cuda(), _codes_dev(codes), buf[:, :N], B, Lq)
    torch.cuda.synchronize()
    assert (buf[:, N:] == GUARD).all(), "columns past N were written"
    return buf[:, :N].cpu().numpy()


def _exact(shape, route=None):
    from polus_amd import ops
    B, N, Lq, Ld, K = shape
    want_route = "lds" if (K + 1) * Lq * 4 <= LDS_BYTES else "global"
    assert route in (None, want_route) and ops.centroid_scores_route(B, N, Lq, Ld, K).route == want_route, shape
    table, qmask, codes = score_case(*shape)
    want, _ = cr.centroid_scores(table, qmask, codes, B, Lq)
    assert np.abs(want).max() < 2 ** 24
    got = _scores(table, qmask, codes, B, Lq)
    assert np.array_equal(_bits(got), _bits(want)), (shape, np.argwhere(_bits(got) != _bits(want))[:5].tolist())
    if N > 2 and B > 1:
        assert (got[:, 1] == 0).all() and (got[1] == 0).all() and np.abs(got[0]).max() > 0
    want_nomask, _ = cr.centroid_scores(table, None, codes, B, Lq)
    assert np.array_equal(_bits(_scores(table, None, codes, B, Lq)), _bits(want_nomask)), shape


@pytest.mark.parametrize("shape", SCORE_SHAPES)
def test_scores_exact_on_integer_tables(shape):
    """Integers in [-8, 8]: every sum is an integer below 2^24, so any order gives the reference's bits.  All but the
    fourth shape (K = 1000 at Lq = 64: 250 KiB) take the LDS route."""
    _exact(shape)


@pytest.mark.parametrize("shape", GLOBAL_SHAPES)
def test_scores_exact_on_the_global_route(shape):
    _exact(shape, "global")


def test_scores_exact_on_both_sides_of_the_route_boundary():
    from polus_amd import ops
    lo, hi = 1, 65535                                                  # the largest K on the LDS route at Lq = 32
    assert ops.centroid_scores_route(2, 40, 32, 70, lo).route == "lds" and ops.centroid_scores_route(2, 40, 32, 70, hi).route == "global"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ops.centroid_scores_route(2, 40, 32, 70, mid).route == "lds" else (lo, mid)
    assert (lo + 1) * 32 * 4 <= LDS_BYTES < (lo + 2) * 32 * 4
    assert ops.centroid_scores_route(2, 40, 32, 70, lo) == ("lds", (lo + 1) * 32 * 4)
    _exact((2, 40, 32, 70, lo), "lds")
    _exact((2, 40, 32, 70, lo + 1), "global")


@pytest.mark.parametrize("shape", [SCORE_SHAPES[2], SCORE_SHAPES[4], GLOBAL_SHAPES[1]])
def test_scores_do_not_depend_on_the_launch(shape):
    """N(0, 1) tables, where an order of summation would show: an entry has the same bits from the full launch, from a
    launch with a subset of the queries and from one with a subset of the documents."""
    B, N, Lq, Ld, K = shape
    table, qmask, codes = score_case(*shape, integer=False)
    qmask[1] = qmask[0]                                                # no empty query here: every row carries bits
    full = _scores(table, qmask, codes, B, Lq)
    b0, b1 = 1, B
    sub_q = _scores(np.ascontiguousarray(table[:, b0 * Lq:b1 * Lq]), qmask[b0:b1], codes, b1 - b0, Lq)
    assert np.array_equal(_bits(sub_q), _bits(full[b0:b1]))
    n0, n1 = N // 3, N - 2
    sub_d = _scores(table, qmask, codes[n0:n1], B, Lq)
    assert np.array_equal(_bits(sub_d), _bits(full[:, n0:n1]))
    one = _scores(table, qmask, codes[N - 1:], B, Lq)
    assert np.array_equal(_bits(one), _bits(full[:, N - 1:]))
    assert np.array_equal(_bits(_scores(table, qmask, codes, B, Lq)), _bits(full))        # and from run to run


@pytest.mark.parametrize("shape", SCORE_SHAPES + GLOBAL_SHAPES)
def test_scores_against_float64_on_normal_tables(shape):
    """The maxima are exact, so only the f32 sum of the Lq terms rounds: in any order
    |got - ref| <= (Lq - 1) * 2^-24 * sum |term| to first order; 1.01 covers the higher orders."""
    B, N, Lq, Ld, K = shape
    table, qmask, codes = score_case(*shape, integer=False)
    want, mag = cr.centroid_scores(table, qmask, codes, B, Lq)
    got = _scores(table, qmask, codes, B, Lq).astype(np.float64)
    bound = 1.01 * (Lq - 1) * 2.0 ** -24 * mag
    worst = float((np.abs(got - want) / np.maximum(bound, 1e-300)).max()) if Lq > 1 else 0.0
    print(f"{shape}: worst |got - ref| / bound = {worst:.3f}")
    assert (np.abs(got - want) <= bound).all(), shape


@pytest.mark.parametrize("rows,K", CODE_SHAPES)
def test_codes_exact(rows, K):
    from polus_amd import ops
    sim, mask = code_case(rows, K)
    want = cr.centroid_codes(sim[:, :K], mask)
    s = torch.as_tensor(sim).cuda()
    for m in (mask, None):
        out = torch.full((rows + 8,), 1234, dtype=torch.int16, device="cuda")
        ops.centroid_codes(s[:, :K], None if m is None else torch.as_tensor(m).cuda(), out, rows=rows)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[rows:] == 1234).all(), "codes past the rows were written"
        ref = want if m is not None else cr.centroid_codes(sim[:, :K], None)
        assert np.array_equal(got[:rows].view(np.uint16), ref), (rows, K, m is None)
    if rows >= 3:
        assert want[rows - 1] == 0 and want[rows - 2] == NONE          # the all-NaN row and the masked row
    # an offset view: rows start at every 4-byte phase of a 16-byte line
    wide = torch.full((rows, K + 9), float("inf"), dtype=torch.float32, device="cuda")
    wide[:, 1:1 + K] = s[:, :K]
    out = torch.empty((rows,), dtype=torch.int16, device="cuda")
    ops.centroid_codes(wide[:, 1:1 + K], torch.as_tensor(mask).cuda(), out)
    assert np.array_equal(out.cpu().numpy().view(np.uint16), want)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("T,K,E", UPDATE_SHAPES)
def test_update_counts_exact_centroids_within_the_derived_bound(T, K, E, mode):
    """Bound on out = s / |s| against float64 over the inputs as the device sees them, u = 2^-24:
      the f32 sum of n rows in any order errs by es <= 1.01 (n - 1) u sum|x| per feature;
      |s| is off by at most |es|_2, and its own f32 evaluation (E squares and E - 1 adds, a square root) by
      (E / 2 + 2) u relative; the division adds u and the rounding to dtype ud = 2^-24 (f32) or 2^-8 (bf16: 8
      significant bits, half a unit in the last place), so
      |out - ref| <= es / |s| + |ref| (|es|_2 / |s| + 1.01 (E + 4) u + ud)."""
    from polus_amd import ops
    x, codes, prev = update_case(T, K, E)
    dt = DT[mode]
    xd, pd = torch.as_tensor(x).to(dt).cuda(), torch.as_tensor(prev).to(dt).cuda()
    want, counts, sums, mags = cr.centroid_update(rounded(x, dt), codes, rounded(prev, dt))
    outs = []
    for _ in range(2):
        out = torch.full((K, E), 99.0, dtype=dt, device="cuda")
        cnt = torch.full((K,), -5, dtype=torch.int32, device="cuda")
        ops.centroid_update(xd, _codes_dev(codes), pd, out, cnt)
        torch.cuda.synchronize()
        outs.append(out)
        assert np.array_equal(cnt.cpu().numpy(), counts)
    assert torch.equal(outs[0].view(torch.int16 if mode == "bf16" else torch.int32),
                       outs[1].view(torch.int16 if mode == "bf16" else torch.int32)), "two launches differ"
    got = outs[0].float().cpu().numpy().astype(np.float64)
    u, ud = 2.0 ** -24, (2.0 ** -24 if mode == "f32" else 2.0 ** -8)
    worst = 0.0
    for k in range(K):
        nrm = np.sqrt((sums[k] ** 2).sum())
        if counts[k] == 0 or nrm == 0:
            assert np.array_equal(got[k], rounded(prev, dt)[k]), f"centroid {k} should keep prev"
            continue
        es = 1.01 * (counts[k] - 1) * u * mags[k]
        bound = es / nrm + np.abs(want[k]) * (np.linalg.norm(es) / nrm + 1.01 * (E + 4) * u + ud)
        worst = max(worst, float((np.abs(got[k] - want[k]) / bound).max()))
        assert (np.abs(got[k] - want[k]) <= bound).all(), (k, counts[k])
    print(f"T={T} K={K} E={E} {mode}: worst |out - ref| / bound = {worst:.3f}")
    if K >= 5 and T >= 20:
        assert counts[0] > T // 2 and counts[K - 1] == 0 and counts[1] == 8 and (sums[1] == 0).all()
