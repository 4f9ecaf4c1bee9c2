"""GPU: every kernel of the MaxSim family at E / 32 = 3, 5, 6, 7, on the in-register route and on the rounds route
(tests/maxsim_ks_cases.py).  polus_maxsim_scores is held to the float64 reference at tests/maxsim_cases.TOL; everything
else is chained to it bit for bit, as in the suites of the single kernels: the rerank, the FP8 scores and rerank, the
residual rerank, and the tuple forward (score and argmax) against polus_maxsim_fwd."""
import numpy as np
import pytest
import torch

from tests import maxsim_ks_cases as ks
from tests import maxsim_ref
from tests.maxsim_cases import TOL
from tests.rerank_cases import candidates, make_case, present
from tests.residual_cases import gaussian_case
from tests.tuple_ref import doc_rows
from tests.util import assert_close, dev, host, relerr, rounded

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
NAN = float("nan")


def _same_bits(got, want, what):
    torch.cuda.synchronize()
    got, want = got.view(torch.int32), want.view(torch.int32)
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {got.numel()} entries differ"


def _at(full, cand_t, ok_t):
    """full[b, cand[b, c]] where the candidate is present, -inf elsewhere."""
    return torch.where(ok_t, full.gather(1, torch.where(ok_t, cand_t, 0).long()), torch.tensor(-np.inf, device="cuda"))


@pytest.mark.parametrize("Lq", ks.LQS)
@pytest.mark.parametrize("mode", ks.MODES)
@pytest.mark.parametrize("E", ks.ES)
def test_every_kernel_of_the_family_agrees(E, mode, Lq):
    from polus_amd import ops
    shape = ks.shape(E, Lq)
    Q, N, _, Ld, _ = shape
    what = f"E={E} {mode} Lq={Lq} ({ks.route(E, mode, Lq)})"
    q, d, qm, dm = make_case(shape, "ragged")
    qt, dt, qmt, dmt = dev(q, DT[mode]), dev(d, DT[mode]), dev(qm), dev(dm)
    cand = candidates(Q, N, ks.C)
    ok = present(cand, N)
    assert ok.any() and (~ok).any() and (cand[:, 0] == N - 1).all()
    cand_t, ok_t = dev(cand), dev(ok)

    def scores(corpus):
        out = torch.full((Q, N), NAN, dtype=torch.float32, device="cuda")
        ops.maxsim_scores(qt, corpus, qmt, dmt, out)
        return out

    def reranked(fn, *corpus):
        out = torch.full((Q, ks.C), NAN, dtype=torch.float32, device="cuda")
        fn(qt, *corpus, qmt, dmt, cand_t, out)
        return out

    # the corpus scores against float64, on the inputs as the device sees them
    full = scores(dt)
    want = maxsim_ref.maxsim_fwd(rounded(q, DT[mode]), rounded(d, DT[mode]), qm, dm)[0]
    got = host(full)
    print(f"[maxsim ks] {what}: score rel err {relerr(got, want):.3e} (tolerance {TOL[mode]['score']:.1e})")
    assert np.isfinite(got).all() and (got[:, N - 1] == 0).all() and (got[Q - 1] == 0).all() and np.abs(got).max() > 0
    assert_close(got, want, TOL[mode]["score"], f"{what}: polus_maxsim_scores")

    # the rerank: those bits at the present candidates, -inf at the absent ones
    rr = reranked(ops.maxsim_rerank, dt)
    _same_bits(rr, _at(full, cand_t, ok_t), f"{what}: polus_maxsim_rerank")
    assert torch.isneginf(rr[~ok_t]).all() and torch.isfinite(rr[ok_t]).all()

    # the FP8 index: scores of the dequantised corpus, and the rerank of those
    codes = torch.empty(dt.shape, dtype=torch.uint8, device="cuda")
    scale = torch.empty(dt.shape[:2], dtype=torch.float32, device="cuda")
    ops.fp8_quantize(dt, codes, scale)
    deq = torch.empty_like(dt)
    ops.fp8_dequantize(codes, scale, deq)
    f8 = torch.full((Q, N), NAN, dtype=torch.float32, device="cuda")
    ops.maxsim_scores_fp8(qt, codes, scale, qmt, dmt, f8)
    _same_bits(f8, scores(deq), f"{what}: polus_maxsim_scores_fp8")
    _same_bits(reranked(ops.maxsim_rerank_fp8, codes, scale), _at(f8, cand_t, ok_t), f"{what}: polus_maxsim_rerank_fp8")

    # the residual index: the rerank of the decompressed corpus
    rq, rqm, rdm, rcodes, packed, cent, w = gaussian_case(shape, "ragged", ks.K, ks.NBITS, mode)
    assert np.array_equal(rq, q) and np.array_equal(rqm, qm) and np.array_equal(rdm, dm)
    rc, rp, rcent, rw = dev(rcodes), dev(packed), dev(cent, DT[mode]), dev(w)
    dec = torch.empty_like(dt)
    ops.residual_decompress(rc, rp, rcent, rw, ks.NBITS, dec)
    res = torch.full((Q, ks.C), NAN, dtype=torch.float32, device="cuda")
    ops.maxsim_rerank_res(qt, rc, rp, rcent, rw, ks.NBITS, qmt, dmt, cand_t, res)
    _same_bits(res, reranked(ops.maxsim_rerank, dec), f"{what}: polus_maxsim_rerank_res")
    assert torch.isfinite(res[ok_t]).all() and res[ok_t].abs().max() > 0

    # the tuple forward, both layouts: the matching entries of polus_maxsim_fwd, score and argmax
    n = ks.TUPLE_N
    fwd = torch.full((Q, N), NAN, dtype=torch.float32, device="cuda")
    fwd_am = torch.full((Q, N, Lq), 12345, dtype=torch.int32, device="cuda")
    ops.maxsim_fwd(qt, dt, qmt, dmt, fwd, fwd_am)
    _same_bits(fwd, full, f"{what}: polus_maxsim_fwd against polus_maxsim_scores")
    b_t = torch.arange(Q, device="cuda")[:, None]
    for layout in (0, 1):
        rows_t = dev(doc_rows(Q, n, layout))
        score = torch.full((Q, n), NAN, dtype=torch.float32, device="cuda")
        am = torch.full((Q, n, Lq), 12345, dtype=torch.int32, device="cuda")
        ops.maxsim_tuples_fwd(qt, dt, qmt, dmt, score, am, layout)
        _same_bits(score, fwd[b_t, rows_t], f"{what}: polus_maxsim_tuples_fwd layout {layout}, score")
        assert torch.equal(am, fwd_am[b_t, rows_t]), f"{what}: polus_maxsim_tuples_fwd layout {layout}, argmax"
        assert ((am >= -1) & (am < Ld)).all() and (am >= 0).any()
