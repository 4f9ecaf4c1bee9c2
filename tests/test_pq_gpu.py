"""GPU: the product-quantisation kernels bit for bit against tests/pq_ref.py on the cases of tests/pq_cases.py, then
CorpusIndex.fit_pq, the PQ index (exact on the planted integer corpus, within the dot tolerance of float64 on N(0, 1) data)
and its place under TwoStageSearch and HybridSearch.  Inputs and outputs are views of wider poisoned buffers whose surplus
must come back untouched, inputs must be unchanged, and every check prints its figure."""
import numpy as np
import pytest
import torch

from tests import fusion_ref as fr
from tests import pq_cases as pc
from tests import pq_ref as pr
from tests import search_ref as sr
from tests.search_cases import CLS_CASE, KS, TableModel, batches, cls_case, dot_tol, token_case
from tests.util import rounded

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
FSENT = -9.25                  # outputs are pre-filled with it
POISON_CODE = 1                # a valid code: reading the surplus of a code buffer would change the result
POISON_X = 1e6


def _wide(a, extra_rows, extra_cols, fill, dtype=None):
    """(buffer, view): the host array a [R, C] inside a device buffer [R + extra_rows, C + extra_cols] of `fill`."""
    t = torch.as_tensor(np.ascontiguousarray(a))
    t = t if dtype is None else t.to(dtype)
    buf = torch.full((a.shape[0] + extra_rows, a.shape[1] + extra_cols), fill, dtype=t.dtype).cuda()
    view = buf[:a.shape[0], :a.shape[1]]
    view.copy_(t)
    return buf, view


def _out(rows, cols, extra_cols, dtype, fill):
    buf = torch.full((rows + 1, cols + extra_cols), fill, dtype=dtype, device="cuda")
    return buf, buf[:rows, :cols]


def _untouched(buf, rows, cols, fill):
    h = buf.float().cpu().numpy() if buf.dtype == torch.bfloat16 else buf.cpu().numpy()
    return bool((h[rows:] == fill).all() and (h[:rows, cols:] == fill).all())


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a.astype(np.float32, copy=False)).view(np.int32)


def _same_bits(got, want, what):
    """Equal bits; a NaN matches any NaN (the payload of a generated NaN is the hardware's)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs in other places"
    diff = int((_bits(got)[~nan] != _bits(want)[~nan]).sum())
    assert diff == 0, f"{what}: {diff} of {got.size} values differ in bits"


def _np(pair):
    torch.cuda.synchronize()
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), f"{what}: ids differ in {int((got[1] != want[1]).sum())} places"
    assert np.array_equal(_bits(got[0]), _bits(want[0])), f"{what}: values differ"


# ---------------------------------------------------------------- the scan
def _scan(table, codes, pad_codes=16, pad_score=5):
    """One polus_pq_scores launch on strided views with poisoned surroundings; returns the host scores."""
    from polus_amd import ops
    Q, N = table.shape[0], codes.shape[0]
    lut = torch.as_tensor(table).cuda()
    bc, cv = _wide(codes, 1, pad_codes, POISON_CODE)
    before = (lut.clone(), bc.clone())
    bs, score = _out(Q, N, pad_score, torch.float32, FSENT)
    ops.pq_scores(lut, cv, score)
    torch.cuda.synchronize()
    assert _untouched(bs, Q, N, FSENT), "wrote outside the [Q, N] scores"
    assert torch.equal(lut.view(torch.int32), before[0].view(torch.int32)) and torch.equal(bc, before[1]), "an input changed"
    return score.cpu().numpy()


@pytest.mark.parametrize("m,ksub", pc.SCAN_FORMATS)
def test_scores_match_the_reference_bit_for_bit(m, ksub):
    from polus_amd import ops
    qts = set()
    for Q in pc.SCAN_Q:
        qt = ops.pq_scores_route(Q, 1000, m, ksub).qt
        qts.add((Q, qt))
        for N in pc.SCAN_N:
            table, codes = pc.scan_case(m, ksub, Q, N)
            want = pr.scores(table, codes)
            for pad in (16, 3, 0):                              # 16-byte pieces where m allows, single bytes, 4-byte pieces
                _same_bits(_scan(table, codes, pad_codes=pad), want, f"m {m} ksub {ksub} Q {Q} N {N} ldc {m + pad}")
    assert any(Q % qt for Q, qt in qts) or m * 1024 * 2 > 160 * 1024, qts      # a tail group wherever qt > 1 fits
    print(f"[pq] scores m {m} ksub {ksub}: (Q, qt) {sorted(qts)}, N {pc.SCAN_N}, ldc m + (16, 3, 0): all bits equal")


def test_scores_of_foreign_codes_special_tables_and_chunks():
    m, ksub, Q, N = 20, 16, 5, 1000
    table, codes = pc.scan_case(m, ksub, Q, N, seed=1)
    foreign = np.arange(3, N, 97)
    codes[foreign, foreign % m] = np.where(foreign % 2, 16, 255).astype(np.uint8)
    table[1, 2, 7], table[2, 0, 1], table[3] = np.nan, -np.inf, -0.0
    table[4, 5, 3] = np.inf
    want = pr.scores(table, codes)
    got = _scan(table, codes)
    _same_bits(got, want, "special values")
    assert (got[0, foreign] == -np.inf).all() and (np.delete(got[0], foreign) > -np.inf).all()
    assert np.isnan(got[1]).any() and (got[2] == -np.inf).sum() > len(foreign)
    ok = np.delete(got[3], foreign)
    assert (ok == 0).all() and not np.signbit(ok).any()          # +0.0 + -0.0 = +0.0
    parts = np.concatenate([_scan(table, codes[a:b]) for a, b in ((0, 1), (1, 640), (640, N))], axis=1)
    _same_bits(parts, got, "three chunks against one launch")
    rows = np.concatenate([_scan(table[b:b + 1], codes) for b in range(Q)])
    _same_bits(rows, got, "one query per launch against five")
    print(f"[pq] {len(foreign)} documents with a byte >= ksub score -inf; NaN, -inf, +inf and -0.0 entries propagate as IEEE says; "
          "1 launch == 3 chunks == 5 single-query launches in bits")


# ---------------------------------------------------------------- lut, encode, decode
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("dsub", pc.DSUBS)
def test_lut_encode_decode_match_the_reference(dsub, mode):
    from polus_amd import ops
    m, ksub, E = 8, 37, 8 * dsub
    cb = pc.codebook(m, ksub, dsub)
    cb[3, 9] = cb[3, 4]                                       # an exact tie: the lower code wins
    cb[1, 0, 0] = np.nan                                      # a codeword at NaN distance from everything: never chosen
    dcb = torch.as_tensor(cb).cuda()
    for rows in pc.ROWS:
        r = pc.rng(100 + rows + dsub)
        x = r.standard_normal((rows, E)).astype(np.float32)
        x[0, 3 * dsub:4 * dsub] = cb[3, 4]
        x[rows - 1, 5 * dsub] = np.nan                        # all distances NaN: code 0
        xr = rounded(x, DT[mode]).astype(np.float32)
        bx, xv = _wide(x, 1, 3, POISON_X, DT[mode])
        keep = bx.clone()
        # lut
        lut = torch.full((rows, m, ksub), FSENT, dtype=torch.float32, device="cuda")
        ops.pq_lut(xv, dcb, lut)
        _same_bits(lut.cpu().numpy(), pr.lut(xr, cb), f"lut dsub {dsub} rows {rows} {mode}")
        # encode
        bcodes, codes = _out(rows, m, 5, torch.uint8, 77)
        ops.pq_encode(xv, dcb, codes)
        torch.cuda.synchronize()
        want = pr.encode(xr, cb)
        got = codes.cpu().numpy()
        assert np.array_equal(got, want), f"encode dsub {dsub} rows {rows} {mode}: {int((got != want).sum())} codes differ"
        assert _untouched(bcodes, rows, m, 77) and torch.equal(bx.view(torch.int16 if mode == "bf16" else torch.int32),
                                                               keep.view(torch.int16 if mode == "bf16" else torch.int32))
        assert (got[:, 3] != 9).all() and (mode == "bf16" or got[0, 3] == 4)      # f32: the planted sub-vector is codeword 4 = 9
        assert got[rows - 1, 5] == 0 and (got[:, 1] != 0).all()
        # decode, with a foreign code
        c = want.copy()
        c[0, 2] = 255 if ksub < 256 else c[0, 2]
        bc, cv = _wide(c, 1, 3, POISON_CODE)
        by, y = _out(rows, E, 2, DT[mode], FSENT)
        ops.pq_decode(cv, dcb, y)
        torch.cuda.synchronize()
        ref = torch.as_tensor(pr.decode(c, cb)).to(DT[mode]).float().numpy()
        _same_bits(y.float().cpu().numpy(), ref, f"decode dsub {dsub} rows {rows} {mode}")
        assert _untouched(by, rows, E, FSENT) and (y[0, 2 * dsub:3 * dsub] == 0).all()
    print(f"[pq] lut / encode / decode, dsub {dsub}, {mode}, rows {pc.ROWS}: bits and codes equal; tie -> 4, all-NaN -> 0, foreign -> zeros")


def test_encode_tie_goes_to_the_lower_code():
    from polus_amd import ops
    p = pc.planted()
    cb = p["cb"].copy()
    cb[:, 11] = cb[:, 2]                                      # codeword 11 repeats 2 in every sub-space
    x = pr.decode(np.full((65, 8), 11, np.uint8), cb)
    for mode in ("f32", "bf16"):
        codes = torch.full((65, 8), 77, dtype=torch.uint8, device="cuda")
        ops.pq_encode(torch.as_tensor(x).to(DT[mode]).cuda(), torch.as_tensor(cb).cuda(), codes)
        assert (codes == 2).all(), mode


# ---------------------------------------------------------------- update
@pytest.mark.parametrize("T", pc.UPDATE_T)
def test_update_matches_the_reference(T):
    from polus_amd import ops
    m, ksub, dsub = 8, 16, 4
    r = pc.rng(200 + T)
    x = r.standard_normal((T, m * dsub)).astype(np.float32)
    codes = r.integers(0, ksub, size=(T, m)).astype(np.uint8)
    codes[codes[:, 2] == 5, 2] = 6                            # an empty cluster: (2, 5) keeps prev
    codes[::7, 4] = 200                                       # codes >= ksub are skipped
    prev = pc.codebook(m, ksub, dsub, seed=9)
    for mode in ("f32", "bf16"):
        xr = rounded(x, DT[mode]).astype(np.float32)
        want, want_counts = pr.update(xr, codes, prev)
        bx, xv = _wide(x, 1, 3, POISON_X, DT[mode])
        bc, cv = _wide(codes, 1, 5, POISON_CODE)
        keep = (bx.clone(), bc.clone())
        dprev = torch.as_tensor(prev).cuda()
        out = torch.full((m, ksub, dsub), FSENT, dtype=torch.float32, device="cuda")
        counts = torch.full((m, ksub), -77, dtype=torch.int32, device="cuda")
        ops.pq_update(xv, cv, dprev, out, counts)
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), want_counts), f"T {T} {mode}: counts"
        _same_bits(out.cpu().numpy(), want, f"update T {T} {mode}")
        assert torch.equal(bc, keep[1]) and torch.equal(bx.float(), keep[0].float()) and torch.equal(dprev.cpu(), torch.as_tensor(prev))
        assert want_counts[2, 5] == 0 and np.array_equal(_bits(out[2, 5]), _bits(prev[2, 5]))
        assert want_counts[4].sum() == T - len(range(0, T, 7))
        out2 = torch.empty_like(out)
        ops.pq_update(xv, cv, dprev, out2, counts)
        assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    print(f"[pq] update T {T}: counts exact ({int(want_counts.sum())} of {T * m} coded, cluster (2, 5) empty keeps prev), centroid bits equal, twice")


# ---------------------------------------------------------------- fit_pq and the index
def _plain(case, mode, **kw):
    from polus_amd.ir.search import CorpusIndex
    from polus_amd.ir.training import InBatchDotScores
    index = CorpusIndex(TableModel(case["table"], DT[mode], False), InBatchDotScores(), **kw)
    n = len(case["d_ids"])
    for b in batches(case["d_ids"], case["d_mask"], [n // 2, n - n // 2]):
        index.add(b)
    return index, {"input_ids": case["q_ids"], "attention_mask": case["q_mask"]}


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_fit_pq_is_the_reference_loop_bit_for_bit(mode):
    f = pc.FIT
    c = cls_case(f["seed"], 4, f["N"], f["E"])
    index, _ = _plain(c, mode)
    codec = index.fit_pq(f["m"], f["ksub"], iters=f["iters"], sample=f["sample"], seed=3)
    docs = rounded(c["table"][c["d_ids"][:, 0]], DT[mode]).astype(np.float32)
    rows = pr.sample_rows(f["N"], f["sample"], 3)
    assert len(rows) == f["sample"] < f["N"]
    want = pr.fit(docs[rows], f["m"], f["ksub"], f["iters"])
    assert (codec.m, codec.ksub, codec.dsub, codec.E) == (f["m"], f["ksub"], f["E"] // f["m"], f["E"])
    _same_bits(codec.codebooks.cpu().numpy(), want, f"fit_pq {mode}")
    again = index.fit_pq(f["m"], f["ksub"], iters=f["iters"], sample=f["sample"], seed=3)
    assert torch.equal(codec.codebooks.view(torch.int32), again.codebooks.view(torch.int32))
    other = index.fit_pq(f["m"], f["ksub"], iters=f["iters"], sample=f["sample"], seed=4)
    assert not torch.equal(codec.codebooks, other.codebooks)
    whole = index.fit_pq(f["m"], f["ksub"], iters=1, sample=1 << 16, seed=3)                 # N <= sample: a permutation
    _same_bits(whole.codebooks.cpu().numpy(), pr.fit(docs[pr.sample_rows(f["N"], 1 << 16, 3)], f["m"], f["ksub"], 1), "whole corpus")
    print(f"[pq] fit_pq {mode}: {f['iters']} rounds over {f['sample']} of {f['N']} vectors equal the reference loop in bits; same seed, same bits")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_pq_index_is_exact_on_the_planted_corpus(mode):
    from polus_amd.ir.search import CorpusIndex, PQCodec
    from polus_amd.ir.training import InBatchDotScores
    p = pc.planted()
    c = pc.as_search_case(p["q"], p["docs"])
    Q, N, m = len(p["q"]), len(p["docs"]), p["cb"].shape[0]
    plain, queries = _plain(c, mode, scratch_bytes=4 * Q * 300)
    index = CorpusIndex(TableModel(c["table"], DT[mode], False), InBatchDotScores(), scratch_bytes=4 * Q * 300, storage="pq",
                        codec=PQCodec(p["cb"]))
    ids = [index.add(b) for b in batches(c["d_ids"], c["d_mask"], [N // 2, N - N // 2])]
    assert torch.cat(ids).cpu().tolist() == list(range(N)) and len(index) == N and len(index.chunks(Q)) == 3
    assert index.pq_codes.dtype == torch.uint8 and np.array_equal(index.pq_codes.cpu().numpy(), p["codes"])
    assert index.nbytes == N * m and index.representations.dtype == DT[mode]
    assert np.array_equal(index.representations.float().cpu().numpy(), p["docs"])
    exact = p["q"].astype(np.float64) @ p["docs"].astype(np.float64).T
    for k in KS:
        got = _np(index.search(queries, k))
        _same(got, _np(plain.search(queries, k)), f"planted {mode} k={k}: PQ against the plain index")
        _same(got, sr.topk(exact.astype(np.float32), k), f"planted {mode} k={k}: PQ against float64")
    ties = [N - len(np.unique(row)) for row in exact]
    print(f"[pq] planted corpus {mode}: codes are the planted ones; search over 3 chunks equals the plain [CLS] index and float64 "
          f"in ids and bits for k {KS}; tied scores per query {ties}; {index.nbytes} bytes against {plain.nbytes}")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_pq_index_search_against_float64_of_the_decoded_vectors(mode):
    """N(0, 1) data, codec from fit_pq.  The float64 reference is the dot product of the (rounded) query with the DECODED
    vector, the f32 codewords its codes name (tests/pq_ref.decode): quantisation error is deliberately outside this test.  On a
    bf16 index `representations` rounds those codewords once more to bf16, which `search` does not (its table is built from
    the f32 codebook), so the reference decodes in f32.  Tolerance: tests/search_cases.dot_tol(E) * max|score|, no case excused."""
    from polus_amd.ir.search import CorpusIndex
    from polus_amd.ir.training import InBatchDotScores
    c = cls_case(**CLS_CASE)
    E = CLS_CASE["E"]
    plain, queries = _plain(c, mode)
    codec = plain.fit_pq(16, 256, iters=2, sample=2048, seed=0)
    index = CorpusIndex(TableModel(c["table"], DT[mode], False), InBatchDotScores(), storage="pq", codec=codec)
    for b in batches(c["d_ids"], c["d_mask"], [2000, 3000]):
        index.add(b)
    cb = codec.codebooks.cpu().numpy()
    codes = index.pq_codes.cpu().numpy()
    docs = rounded(c["table"][c["d_ids"][:, 0]], DT[mode]).astype(np.float32)
    assert np.array_equal(codes, pr.encode(docs, cb))
    decoded = pr.decode(codes, cb)
    want_reps = torch.as_tensor(decoded).to(DT[mode]).float().numpy()
    assert np.array_equal(_bits(index.representations.float()), _bits(want_reps))
    s64 = sr.dot_scores(rounded(c["table"][c["q_ids"][:, 0]], DT[mode]), decoded)
    t = dot_tol(E) * np.abs(s64).max()
    rel = float(np.linalg.norm(decoded - docs) / np.linalg.norm(docs))
    for k in KS:
        val, idx = _np(index.search(queries, k))
        worst = max(np.abs(val[r].astype(np.float64) - s64[r, idx[r]]).max() for r in range(len(idx)))
        print(f"[pq] N(0, 1) {mode} k={k}: worst |score - float64 over decoded| = {worst:.3e}, t = {t:.3e} "
              f"(quantiser: relative L2 error {rel:.3f}, outside this test)")
        assert sr.check_against_float64(val, idx, s64, k, t) == []


def test_pq_index_under_two_stage_and_hybrid_search():
    from polus_amd.ir.fusion import HybridSearch
    from polus_amd.ir.search import CorpusIndex, TwoStageSearch
    from polus_amd.ir.training import InBatchDotScores, MaxSimScores
    c = token_case(seed=3, Q=8, N=300, Lq=8, Ld=12, E=32, V=512)
    N, Q = 300, 8
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    plain, _ = _plain(c, "f32")
    codec = plain.fit_pq(8, 32, iters=2)
    pq = CorpusIndex(TableModel(c["table"], torch.float32, False), InBatchDotScores(), storage="pq", codec=codec)
    token = CorpusIndex(TableModel(c["table"], torch.float32, True), MaxSimScores(normalize=False))
    two = TwoStageSearch(pq, token, candidates=50)
    for b in batches(c["d_ids"], c["d_mask"], [100, 200]):
        two.add(b)
    assert len(two) == len(pq) == len(token) == N
    got = _np(two.search(queries, 10))
    first_ids = pq.search(queries, 50)[1]
    _same(got, _np(token.rerank(queries, first_ids, 10)), "two stages by hand")
    assert all(set(row.tolist()) <= set(f.tolist()) for row, f in zip(got[1], first_ids.cpu().numpy()))
    _same(_np(TwoStageSearch(pq, token, candidates=N).search(queries, 10)), _np(token.search(queries, 10)), "candidates = N")
    # HybridSearch over the PQ index and the plain one: the reference fusion of the two stages' own lists
    depth, k = 40, 10
    hybrid = HybridSearch([pq, plain], depth, weights=[1.0, 0.5])
    own = [s.search(queries, depth) for s in (pq, plain)]
    ids, scores = np.stack([i.cpu().numpy() for _, i in own]), np.stack([s.cpu().numpy() for s, _ in own])
    differ = int((ids[0] != ids[1]).sum())
    for method in ("rrf", "sum"):
        hybrid.method = method
        want_id, want_val, _ = fr.fuse_lists(ids, scores, N, method, [1.0, 0.5], 60.0)
        _same(_np(hybrid.search(queries, k)), fr.topk(want_id, want_val, k), f"hybrid {method}")
    print(f"[pq] TwoStageSearch(pq, token) equals rerank by hand and, at candidates = N, the token search; HybridSearch([pq, plain]) "
          f"equals the reference fusion ({differ} of {ids[0].size} list positions differ between the stages)")


def test_pq_index_refusals():
    from polus_amd.ir.search import CorpusIndex, PQCodec
    from polus_amd.ir.training import InBatchDotScores, MaxSimScores
    p = pc.planted()
    c = pc.as_search_case(p["q"], p["docs"][:40])
    docs = {"input_ids": c["d_ids"], "attention_mask": c["d_mask"]}
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    tok = CorpusIndex(TableModel(c["table"], torch.float32, True), MaxSimScores(normalize=False), storage="pq", codec=PQCodec(p["cb"]))
    with pytest.raises(ValueError, match=r"single \(\[CLS\]\) vectors only"):
        tok.add(docs)
    narrow = CorpusIndex(TableModel(c["table"], torch.float32, False), InBatchDotScores(), storage="pq", codec=PQCodec(p["cb"][:4]))
    with pytest.raises(ValueError, match="quantises vectors of 16 features"):
        narrow.add(docs)
    index = CorpusIndex(TableModel(c["table"], torch.float32, False), InBatchDotScores(), storage="pq", codec=PQCodec(p["cb"]))
    index.add(docs)
    with pytest.raises(ValueError, match=r"\[CLS\]"):
        index.rerank(queries, np.zeros((5, 1), np.int64), 1)
    for call in (lambda: index.fit_centroids(4), lambda: index.set_centroids(np.zeros((4, 32), np.float32))):
        with pytest.raises(ValueError, match=r"\[CLS\]"):
            call()
    with pytest.raises(ValueError, match="needs centroids"):
        index.search_pruned(queries, 3, 10)
    with pytest.raises(ValueError, match="plain \\[CLS\\] index"):
        index.fit_pq(8, 16)
    token = CorpusIndex(TableModel(c["table"], torch.float32, True), MaxSimScores(normalize=False))
    token.add(docs)
    with pytest.raises(ValueError, match="plain \\[CLS\\] index"):
        token.fit_pq(8, 16)
    plain = CorpusIndex(TableModel(c["table"], torch.float32, False), InBatchDotScores())
    plain.add(docs)
    with pytest.raises(ValueError, match="must divide"):
        plain.fit_pq(12, 16)
    with pytest.raises(ValueError, match="at least as many sampled documents"):
        plain.fit_pq(8, 41)
    val, idx = _np(index.search(queries, 100))                 # fewer than k documents: the tail is (-inf, -1)
    assert (idx[:, 40:] == -1).all() and (val[:, 40:] == -np.inf).all() and (idx[:, :40] >= 0).all()
    index.clear()
    assert len(index) == 0 and index.pq_codes is None and index.codec is not None
