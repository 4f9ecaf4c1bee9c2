"""CPU: the cases of tests/maxsim_ks_cases.py reach what they are there for."""
from tests import maxsim_ks_cases as ks
from tests.rerank_cases import candidates, make_case, present


def test_cases_cover_the_ks_no_other_suite_reaches_on_both_routes():
    assert {E // 32 for E in ks.ES} == {3, 5, 6, 7} and all(E % 32 == 0 for E in ks.ES)
    for E in ks.ES:
        for mode in ks.MODES:
            assert 1 <= ks.tiles_per_wave(E, mode) <= 5
            assert ks.route(E, mode, 5) == "registers" and ks.route(E, mode, 100) == "rounds"
    assert set(ks.LQS) == {5, 100} and set(ks.MODES) == {"f32", "bf16"}
    assert (ks.tiles_per_wave(32, "bf16"), ks.tiles_per_wave(32, "f32"), ks.tiles_per_wave(256, "f32")) == (8, 8, 1)
    # three document tiles, the last one partial; the tuples use the whole corpus
    assert -(-ks.LD // 16) == 3 and ks.LD % 16 and ks.Q * ks.TUPLE_N == ks.N


def test_cases_hold_an_empty_document_an_all_masked_query_and_absent_candidates():
    for Lq in ks.LQS:
        q, d, qm, dm = make_case(ks.shape(ks.ES[0], Lq), "ragged")
        assert not dm[ks.N - 1].any() and not qm[ks.Q - 1].any() and dm[:ks.N - 1].any(axis=1).all()
    cand = candidates(ks.Q, ks.N, ks.C)
    ok = present(cand, ks.N)
    assert (cand[:, 0] == ks.N - 1).all() and ok.any(axis=1).all() and (~ok).sum(axis=1).min() >= 4
