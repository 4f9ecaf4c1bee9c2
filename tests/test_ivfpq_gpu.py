"""GPU: the IVF-PQ kernels bit for bit against tests/ivfpq_ref.py on the cases of tests/ivfpq_cases.py, then CorpusIndex.fit_ivfpq,
the IVF-PQ index (exact on the planted integer corpus, exhaustive and probed; within the dot tolerance of float64 on N(0, 1)
data) and its place under TwoStageSearch and HybridSearch.  Inputs and outputs are views of wider poisoned buffers whose surplus
must come back untouched, inputs must be unchanged, and every check prints its figure."""
import numpy as np
import pytest
import torch

from tests import fusion_ref as fr
from tests import ivf_ref
from tests import ivfpq_cases as ic
from tests import ivfpq_ref as ir
from tests import pq_cases as pc
from tests import pq_ref as pr
from tests import search_ref as sr
from tests.search_cases import CLS_CASE, TableModel, batches, cls_case, dot_tol, token_case
from tests.util import rounded

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
FSENT = -9.25                  # outputs are pre-filled with it
POISON_CODE = 1                # a valid code byte: reading the surplus of a code buffer would change the result
POISON_ID = 0                  # a valid id and a valid coarse code
POISON_X = 1e6


def _wide(a, extra_rows, extra_cols, fill, dtype=None):
    """(buffer, view): the host array a [R, C] inside a device buffer [R + extra_rows, C + extra_cols] of `fill`."""
    t = torch.as_tensor(np.ascontiguousarray(a))
    t = t if dtype is None else t.to(dtype)
    buf = torch.full((a.shape[0] + extra_rows, a.shape[1] + extra_cols), fill, dtype=t.dtype).cuda()
    view = buf[:a.shape[0], :a.shape[1]]
    view.copy_(t)
    return buf, view


def _long(a, extra, fill):
    """(buffer, view): the host vector a [R] at the front of a device buffer [R + extra] of `fill`."""
    t = torch.as_tensor(np.ascontiguousarray(a))
    buf = torch.full((a.shape[0] + extra,), fill, dtype=t.dtype).cuda()
    buf[:a.shape[0]].copy_(t)
    return buf, buf[:a.shape[0]]


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


def _i16(coarse):
    return np.asarray(coarse, np.uint16).view(np.int16)


# ---------------------------------------------------------------- the scan
def _scan(lut, cdot, coarse, codes, cand, pad_codes=16, pad_score=5):
    """One polus_ivfpq_scores_ids launch on strided views with poisoned surroundings; returns the host scores [Q, C]."""
    from polus_amd import ops
    Q = lut.shape[0]
    C = codes.shape[0] if cand is None else cand.shape[1]
    dlut = torch.as_tensor(lut).cuda()
    bd, dv = _wide(cdot, 1, 2, POISON_X)
    bo, ov = _long(_i16(coarse), 5, POISON_ID)
    bc, cv = _wide(codes, 1, pad_codes, POISON_CODE)
    bn, nv = (None, None) if cand is None else _wide(cand, 1, 3, POISON_ID)
    before = [t.clone() for t in (dlut.view(torch.int32), bd.view(torch.int32), bo, bc)] + ([] if cand is None else [bn.clone()])
    bs, score = _out(Q, C, pad_score, torch.float32, FSENT)
    ops.ivfpq_scores_ids(dlut, dv, ov, cv, nv, score)
    torch.cuda.synchronize()
    assert _untouched(bs, Q, C, FSENT), "wrote outside the [Q, C] scores"
    after = [dlut.view(torch.int32), bd.view(torch.int32), bo, bc] + ([] if cand is None else [bn])
    assert all(torch.equal(a, b) for a, b in zip(after, before)), "an input changed"
    return score.cpu().numpy()


@pytest.mark.parametrize("m,ksub", ic.SCAN_FORMATS)
def test_scores_match_the_reference_bit_for_bit(m, ksub):
    from polus_amd import ops
    N, routes = ic.SCAN_N, set()
    for Q in ic.SCAN_Q:
        for K in ic.SCAN_K:
            lut, cdot, coarse, codes = ic.scan_case(m, ksub, Q, K)
            full = ir.full_scores(lut, cdot, coarse, codes)                 # the reference once per (Q, K): every pair
            for C in ic.SCAN_C:
                routes.add(tuple(ops.ivfpq_scores_ids_route(Q, C, m, ksub)))
                cand = ic.candidates(Q, C, N, seed=K)
                want = ir.scores_ids(lut, cdot, coarse, codes, cand)
                ok = (cand >= 0) & (cand < N)
                assert np.array_equal(_bits(want[ok]), _bits(full[np.nonzero(ok)[0], cand[ok]])) and (want[~ok] == -np.inf).all()
                for pad in ic.SCAN_PADS:
                    what = f"m {m} ksub {ksub} Q {Q} K {K} C {C} ldc {m + pad}"
                    _same_bits(_scan(lut, cdot, coarse, codes, cand, pad_codes=pad), want, what + " cand")
                    _same_bits(_scan(lut, cdot, coarse[:C], codes[:C], None, pad_codes=pad), full[:, :C], what + " cand=None")
    assert {r[0] for r in routes} == {m * 1024}
    print(f"[ivfpq] scores m {m} ksub {ksub}: Q {ic.SCAN_Q}, K {ic.SCAN_K}, C {ic.SCAN_C} over N {N}, ldc m + {ic.SCAN_PADS}, with "
          f"shuffled candidates (-1, >= N, repeated) and without: all bits equal; (LDS bytes, columns per workgroup) {sorted(routes)}")


def test_scores_of_foreign_codes_special_values_and_chunks():
    from polus_amd import ops
    m, ksub, Q, K, N = 20, 16, 5, 7, 1000
    lut, cdot, coarse, codes = ic.scan_case(m, ksub, Q, K, seed=1)
    no_list = np.arange(5, N, 89)
    coarse[no_list] = np.where(no_list % 2, 0xFFFF, K).astype(np.uint16)
    foreign = np.arange(3, N, 97)
    codes[foreign, foreign % m] = np.where(foreign % 2, 16, 255).astype(np.uint8)
    lut[1, 2, 7], lut[2, 0, 1], lut[3] = np.nan, -np.inf, -0.0
    lut[4, 5, 3] = np.inf
    cdot[0, 3], cdot[1, 1], cdot[2, 2], cdot[3], cdot[4, 0] = np.nan, np.inf, -np.inf, -0.0, -np.inf
    full = ir.full_scores(lut, cdot, coarse, codes)
    cand = ic.candidates(Q, N, N, seed=2)
    want = ir.scores_ids(lut, cdot, coarse, codes, cand)
    got = _scan(lut, cdot, coarse, codes, cand)
    _same_bits(got, want, "special values")
    whole = _scan(lut, cdot, coarse, codes, None)
    _same_bits(whole, full, "special values, cand=None")
    dead = np.union1d(no_list, foreign)
    assert (whole[0, no_list] == -np.inf).all() and (whole[:, no_list] == -np.inf).all()
    live0 = np.delete(whole[0], np.union1d(dead, np.nonzero(coarse == 3)[0]))
    assert (live0 > -np.inf).all() and np.isnan(whole[0, np.setdiff1d(np.nonzero(coarse == 3)[0], dead)]).all()
    assert np.isnan(whole[1]).any() and (whole[2] == -np.inf).sum() > len(dead)
    ok3 = np.delete(whole[3], dead)
    assert (ok3 == 0).all() and not np.signbit(ok3).any()            # -0.0 + (+0.0 + -0.0 ...) = +0.0
    assert np.isnan(whole[4][(codes[:, 5] == 3) & (coarse == 0)]).all()          # -inf + +inf
    # the bits of a pair do not depend on the launch: column chunks, one query per launch, the exhaustive route
    parts = np.concatenate([_scan(lut, cdot, coarse, codes, cand[:, a:b]) for a, b in ((0, 1), (1, 640), (640, N))], axis=1)
    _same_bits(parts, got, "three column chunks against one launch")
    rows = np.concatenate([_scan(lut[b:b + 1], cdot[b:b + 1], coarse, codes, cand[b:b + 1]) for b in range(Q)])
    _same_bits(rows, got, "one query per launch against five")
    ident = np.broadcast_to(np.arange(N, dtype=np.int32), (Q, N)).copy()
    _same_bits(_scan(lut, cdot, coarse, codes, ident), whole, "cand = 0 .. N - 1 against cand=None")
    okc = (cand >= 0) & (cand < N)
    assert np.array_equal(_bits(np.nan_to_num(got[okc], nan=7.0)), _bits(np.nan_to_num(whole[np.nonzero(okc)[0], cand[okc]], nan=7.0)))
    chunks = np.concatenate([_scan(lut, cdot, coarse[a:b], codes[a:b], None) for a, b in ((0, 1), (1, 640), (640, N))], axis=1)
    _same_bits(chunks, whole, "three corpus chunks against one exhaustive launch")
    # with cdot = +0.0 and every document in a list the scores are polus_pq_scores' bits
    zero, in_list = np.zeros((Q, K), np.float32), (coarse % K).astype(np.uint16)
    plain = torch.full((Q, N), FSENT, dtype=torch.float32, device="cuda")
    ops.pq_scores(torch.as_tensor(lut).cuda(), torch.as_tensor(codes).cuda(), plain)
    _same_bits(_scan(lut, zero, in_list, codes, None), plain.cpu().numpy(), "cdot = +0.0 against pq_scores")
    print(f"[ivfpq] {len(no_list)} documents without a list and {len(foreign)} with a byte >= ksub score -inf; NaN, +-inf and -0.0 in "
          "lut and cdot propagate as IEEE says; 1 launch == 3 column chunks == 5 single-query launches == the cand=None scan of the "
          "same pairs (itself == 3 corpus chunks) in bits; with cdot = +0.0 the bits are pq_scores'")


# ---------------------------------------------------------------- residual, coarse update
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("E", ic.RESIDUAL_E)
def test_residual_matches_the_reference(E, mode):
    from polus_amd import ops
    K = 9
    for rows in ic.RESIDUAL_ROWS:
        r = ic.rng(300 + rows + E)
        x, cent = r.standard_normal((rows, E)).astype(np.float32), r.standard_normal((K, E)).astype(np.float32)
        coarse = r.integers(0, K, size=rows).astype(np.uint16)
        coarse[rows - 1] = 0xFFFF if rows > 1 else coarse[0]
        if rows > 2:
            coarse[1] = K
        xr, cr = rounded(x, DT[mode]).astype(np.float32), rounded(cent, DT[mode]).astype(np.float32)
        bx, xv = _wide(x, 1, 3, POISON_X, DT[mode])
        dcent = torch.as_tensor(cent).to(DT[mode]).cuda()
        bo, ov = _long(_i16(coarse), 3, POISON_ID)
        keep = (bx.clone(), dcent.clone(), bo.clone())
        br, rv = _out(rows, E, 2, torch.float32, FSENT)
        ops.ivfpq_residual(xv, dcent, ov, rv)
        torch.cuda.synchronize()
        _same_bits(rv.cpu().numpy(), ir.residual(xr, cr, coarse), f"residual E {E} rows {rows} {mode}")
        assert _untouched(br, rows, E, FSENT)
        assert torch.equal(bx.float(), keep[0].float()) and torch.equal(dcent.float(), keep[1].float()) and torch.equal(bo, keep[2])
        if rows > 2:
            assert (rv[1] == 0).all() and (rv[rows - 1] == 0).all()
    print(f"[ivfpq] residual E {E} {mode}, rows {ic.RESIDUAL_ROWS}: bits equal; coarse codes K and 0xFFFF give zeros")


@pytest.mark.parametrize("T", ic.UPDATE_T)
def test_coarse_update_matches_the_reference(T):
    from polus_amd import ops
    K, E = ic.UPDATE_K, 40                                     # E: two whole chunks of 16 features and a part of a third
    r = ic.rng(400 + T)
    x = r.standard_normal((T, E)).astype(np.float32)
    coarse = r.integers(0, K, size=T).astype(np.uint16)
    coarse[coarse == 5] = 6                                    # an empty cluster keeps prev
    coarse[::7] = np.where(np.arange(0, T, 7) % 2, 0xFFFF, K).astype(np.uint16)        # codes >= K are skipped
    prev = r.standard_normal((K, E)).astype(np.float32)
    for mode in ("f32", "bf16"):
        rt = lambda a: rounded(a, DT[mode]).astype(np.float32)               # noqa: E731
        want, want_counts = ir.coarse_update(rt(x), coarse, rt(prev), rt)
        bx, xv = _wide(x, 1, 3, POISON_X, DT[mode])
        bo, ov = _long(_i16(coarse), 3, POISON_ID)
        dprev = torch.as_tensor(prev).to(DT[mode]).cuda()
        keep = (bx.clone(), bo.clone(), dprev.clone())
        out = torch.full((K, E), FSENT, dtype=DT[mode], device="cuda")
        counts = torch.full((K,), -77, dtype=torch.int32, device="cuda")
        ops.ivfpq_coarse_update(xv, ov, dprev, out, counts)
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), want_counts), f"T {T} {mode}: counts"
        _same_bits(out.float().cpu().numpy(), want, f"coarse update T {T} {mode}")
        assert torch.equal(bx.float(), keep[0].float()) and torch.equal(bo, keep[1]) and torch.equal(dprev.float(), keep[2].float())
        assert want_counts[5] == 0 and np.array_equal(_bits(out[5].float()), _bits(rt(prev)[5]))
        assert want_counts.sum() == T - len(range(0, T, 7))
        out2 = torch.full_like(out, 3.0)
        ops.ivfpq_coarse_update(xv, ov, dprev, out2, counts)
        assert torch.equal(out.float().view(torch.int32), out2.float().view(torch.int32))
    print(f"[ivfpq] coarse update T {T}: counts exact ({int(want_counts.sum())} of {T} in a list, cluster 5 empty keeps prev), "
          "centroid bits equal for f32 and bf16, twice")


# ---------------------------------------------------------------- the index
def _plain(case, mode, **kw):
    from polus_amd.ir.search import CorpusIndex
    from polus_amd.ir.training import InBatchDotScores
    index = CorpusIndex(TableModel(case["table"], DT[mode], False), InBatchDotScores(), **kw)
    n = len(case["d_ids"])
    for b in batches(case["d_ids"], case["d_mask"], [n // 2, n - n // 2]):
        index.add(b)
    return index, {"input_ids": case["q_ids"], "attention_mask": case["q_mask"]}


def _ivfpq(case, mode, codec, sizes, **kw):
    from polus_amd.ir.search import CorpusIndex
    from polus_amd.ir.training import InBatchDotScores
    index = CorpusIndex(TableModel(case["table"], DT[mode], False), InBatchDotScores(), storage="ivfpq", codec=codec, **kw)
    ids = [index.add(b) for b in batches(case["d_ids"], case["d_mask"], sizes)]
    return index, ids


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_ivfpq_index_is_exact_on_the_planted_corpus(mode):
    from polus_amd.ir.search import IVFPQCodec
    p = ic.planted()
    c = pc.as_search_case(p["q"], p["docs"])
    Q, N, K, m = len(p["q"]), len(p["docs"]), len(p["cent"]), p["cb"].shape[0]
    scratch = 4 * Q * 300
    plain, queries = _plain(c, mode, scratch_bytes=scratch)
    index, ids = _ivfpq(c, mode, IVFPQCodec(p["cent"], p["cb"]), [N // 2, N - N // 2], scratch_bytes=scratch)
    assert torch.cat(ids).cpu().tolist() == list(range(N)) and len(index) == N and len(index.chunks(Q)) == 3
    assert index.coarse_codes.dtype == torch.int16 and np.array_equal(index.coarse_codes.cpu().numpy().view(np.uint16), p["coarse"])
    assert index.pq_codes.dtype == torch.uint8 and np.array_equal(index.pq_codes.cpu().numpy(), p["codes"])
    assert index.nbytes == N * (m + 2) and index.representations.dtype == DT[mode] and index.centroids.dtype == DT[mode]
    assert np.array_equal(index.representations.float().cpu().numpy(), p["docs"])
    exact = p["q"].astype(np.float64) @ p["docs"].astype(np.float64).T
    cdot = (p["q"].astype(np.float64) @ p["cent"].astype(np.float64).T).astype(np.float32)
    pro = ir.probes(cdot, 2)
    restricted = ir.probed(exact.astype(np.float32), p["coarse"], pro)
    short = []
    for k in ic.KS:
        got = _np(index.search(queries, k))
        _same(got, _np(plain.search(queries, k)), f"planted {mode} k={k}: IVF-PQ against the plain index")
        _same(got, sr.topk(exact.astype(np.float32), k), f"planted {mode} k={k}: IVF-PQ against float64")
        _same(_np(index.search(queries, k, nprobe=K)), got, f"planted {mode} k={k}: nprobe = K against exhaustive")
        two = _np(index.search(queries, k, nprobe=2))
        _same(two, sr.topk(restricted, k), f"planted {mode} k={k}: nprobe = 2 against the reference over the two best lists")
        for b in range(Q):
            back = two[1][b][two[1][b] >= 0]
            assert set(p["coarse"][back].tolist()) <= set(pro[b].tolist())
        short.append(int((two[1] < 0).sum()))
    assert index.nbytes == N * (m + 2) + 4 * (K + 1) + 4 * N
    ties = [N - len(np.unique(row)) for row in exact]
    sizes = [int((p["coarse"][:, None] == pro[b][None]).any(-1).sum()) for b in range(Q)]
    print(f"[ivfpq] planted corpus {mode}: coarse and PQ codes are the planted ones, representations the documents; search over 3 "
          f"chunks and at nprobe = K = {K} equals the plain [CLS] index and float64 in ids and bits for k {ic.KS} (tied scores per "
          f"query {ties}); nprobe = 2 equals the reference over the two best lists ({sizes} documents per query, padded places "
          f"{short}); {index.nbytes} bytes with lists against {plain.nbytes}")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_ivfpq_index_search_against_float64_of_the_decoded_vectors(mode):
    """N(0, 1) data, codec from fit_ivfpq.  The float64 reference is the dot product of the (rounded) query with the vector the
    index's OWN codes name: its centroid as stored in the index's dtype plus the f32 codewords of its residual codes.
    Quantisation error is deliberately outside this test.  Tolerance: tests/search_cases.dot_tol(E) * max|score|, no case
    excused."""
    c = cls_case(**CLS_CASE)
    E = CLS_CASE["E"]
    plain, queries = _plain(c, mode)
    codec = plain.fit_ivfpq(32, 16, 256, iters=2, pq_iters=2, sample=2048, seed=0)
    assert (codec.K, codec.m, codec.ksub, codec.E) == (32, 16, 256, E) and codec.centroids.dtype == DT[mode]
    index, _ = _ivfpq(c, mode, codec, [2000, 3000])
    cent = index.centroids.float().cpu().numpy().astype(np.float64)
    cb = codec.codebooks.cpu().numpy()
    coarse = index.coarse_codes.cpu().numpy().view(np.uint16)
    codes = index.pq_codes.cpu().numpy()
    assert coarse.max() < 32
    decoded = cent[coarse] + pr.decode(codes, cb).astype(np.float64)
    docs = rounded(c["table"][c["d_ids"][:, 0]], DT[mode])
    s64 = sr.dot_scores(rounded(c["table"][c["q_ids"][:, 0]], DT[mode]), decoded)
    t = dot_tol(E) * np.abs(s64).max()
    rel = float(np.linalg.norm(decoded - docs) / np.linalg.norm(docs))
    used = len(np.unique(coarse))
    for k in ic.KS:
        val, idx = _np(index.search(queries, k))
        worst = max(np.abs(val[r].astype(np.float64) - s64[r, idx[r]]).max() for r in range(len(idx)))
        print(f"[ivfpq] N(0, 1) {mode} k={k}: worst |score - float64 over decoded| = {worst:.3e}, t = {t:.3e} "
              f"(quantiser: relative L2 error {rel:.3f}, {used} of 32 lists used; outside this test)")
        assert sr.check_against_float64(val, idx, s64, k, t) == []


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_fit_ivfpq_is_the_reference_loop_bit_for_bit(mode):
    f, fc = ic.FIT, ic.fit_case()
    rt = lambda a: rounded(a, DT[mode]).astype(np.float32)                   # noqa: E731
    c = pc.as_search_case(fc["docs"][:3], fc["docs"])
    index, _ = _plain(c, mode)
    assert np.array_equal(pr.sample_rows(f["N"], f["sample"], 3), fc["rows"]) and len(fc["rows"]) == f["sample"] < f["N"]
    x = rt(fc["docs"])[fc["rows"]]
    for iters in f["iters"]:
        codec = index.fit_ivfpq(f["K"], f["m"], f["ksub"], iters=iters, pq_iters=f["pq_iters"], sample=f["sample"], seed=3)
        want_cent, want_cb = ir.fit(x, f["K"], f["m"], f["ksub"], iters, f["pq_iters"], rt)
        assert codec.centroids.dtype == DT[mode] and (codec.K, codec.m, codec.ksub, codec.dsub) == (f["K"], f["m"], f["ksub"], 4)
        _same_bits(codec.centroids.float().cpu().numpy(), want_cent, f"fit_ivfpq {mode} iters {iters}: centroids")
        _same_bits(codec.codebooks.cpu().numpy(), want_cb, f"fit_ivfpq {mode} iters {iters}: codebooks")
        assert np.array_equal(codec.half_norms.numpy(), ir.half_norms(want_cent))
    again = index.fit_ivfpq(f["K"], f["m"], f["ksub"], iters=iters, pq_iters=f["pq_iters"], sample=f["sample"], seed=3)
    assert torch.equal(codec.centroids.float().view(torch.int32), again.centroids.float().view(torch.int32))
    assert torch.equal(codec.codebooks.view(torch.int32), again.codebooks.view(torch.int32))
    other = index.fit_ivfpq(f["K"], f["m"], f["ksub"], iters=iters, pq_iters=f["pq_iters"], sample=f["sample"], seed=4)
    assert not torch.equal(codec.codebooks, other.codebooks)
    print(f"[ivfpq] fit_ivfpq {mode}: {f['iters']} coarse rounds and {f['pq_iters']} PQ rounds over {f['sample']} of {f['N']} vectors "
          "equal the reference loop in bits (centroids and codebooks); same seed, same bits; another seed differs")


def test_ivfpq_index_under_two_stage_and_hybrid_search_and_its_lists():
    from polus_amd.ir.fusion import HybridSearch
    from polus_amd.ir.search import CorpusIndex, TwoStageSearch
    from polus_amd.ir.training import MaxSimScores
    c = token_case(seed=3, Q=8, N=300, Lq=8, Ld=12, E=32, V=512)
    N, Q, K, m = 300, 8, 8, 8
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    plain, _ = _plain(c, "f32")
    codec = plain.fit_ivfpq(K, m, 32, iters=2, pq_iters=2)
    token = CorpusIndex(TableModel(c["table"], torch.float32, True), MaxSimScores(normalize=False))
    ivf = CorpusIndex(TableModel(c["table"], torch.float32, False), plain.compute_scores, storage="ivfpq", codec=codec, nprobe=4)
    two = TwoStageSearch(ivf, token, candidates=50)
    for b in batches(c["d_ids"], c["d_mask"], [100, 200]):
        two.add(b)
    assert len(two) == len(ivf) == len(token) == N
    assert ivf.nbytes == N * (m + 2)                                       # no search yet: no lists
    coarse = ivf.coarse_codes.cpu().numpy().view(np.uint16)
    offsets, docs = ivf.lists
    counts, want_off, per = ivf_ref.lists(coarse[:, None], K)
    assert np.array_equal(offsets.cpu().numpy(), want_off) and ivf_ref.split(offsets.cpu(), docs.cpu()) == per
    assert sorted(docs.cpu().tolist()) == list(range(N)) and ivf.nbytes == N * (m + 2) + 4 * (K + 1) + 4 * N
    got = _np(two.search(queries, 10))
    first = ivf.search(queries, 50)
    _same(_np(first), _np(ivf.search(queries, 50, nprobe=4)), "search(queries, k) falls back to the index's nprobe")
    _same(got, _np(token.rerank(queries, first[1], 10)), "two stages by hand")
    fid = first[1].cpu().numpy()
    assert all(set(row.tolist()) <= set(f.tolist()) for row, f in zip(got[1], fid))
    lut_q = ivf.encode_queries(queries)
    cdot = (lut_q.float().cpu().numpy().astype(np.float64) @ ivf.centroids.float().cpu().numpy().astype(np.float64).T)
    pro = ir.probes(cdot.astype(np.float32), 4)
    for b in range(Q):
        assert set(coarse[fid[b][fid[b] >= 0]].tolist()) <= set(pro[b].tolist())
    exhaustive = _np(ivf.search(queries, 50, nprobe=K))
    ivf.nprobe = None
    _same(_np(ivf.search(queries, 50)), exhaustive, "nprobe = K against the exhaustive scan")
    ivf.nprobe = 4
    # HybridSearch over the probed IVF-PQ index and the plain one: the reference fusion of the two stages' own lists
    depth, k = 40, 10
    hybrid = HybridSearch([ivf, plain], depth, weights=[1.0, 0.5])
    own = [s.search(queries, depth) for s in (ivf, plain)]
    ids, scores = np.stack([i.cpu().numpy() for _, i in own]), np.stack([s.cpu().numpy() for s, _ in own])
    differ = int((ids[0] != ids[1]).sum())
    for method in ("rrf", "sum"):
        hybrid.method = method
        want_id, want_val, _ = fr.fuse_lists(ids, scores, N, method, [1.0, 0.5], 60.0)
        _same(_np(hybrid.search(queries, k)), fr.topk(want_id, want_val, k), f"hybrid {method}")
    print(f"[ivfpq] lists: every document in exactly one of {K} lists (sizes {counts.tolist()}), equal to the reference as sets; "
          f"TwoStageSearch(ivfpq(nprobe=4), token) equals rerank by hand, its candidates lie in the probed lists; nprobe = K equals "
          f"the exhaustive scan; HybridSearch([ivfpq, plain]) equals the reference fusion ({differ} of {ids[0].size} list positions "
          "differ between the stages)")


def test_ivfpq_index_refusals_clear_and_short_results():
    from polus_amd.ir.search import CorpusIndex, IVFPQCodec
    from polus_amd.ir.training import InBatchDotScores, MaxSimScores
    p = ic.planted()
    K, m = len(p["cent"]), p["cb"].shape[0]
    c = pc.as_search_case(p["q"], p["docs"][:40])
    docs = {"input_ids": c["d_ids"], "attention_mask": c["d_mask"]}
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    codec = IVFPQCodec(p["cent"], p["cb"])
    tok = CorpusIndex(TableModel(c["table"], torch.float32, True), MaxSimScores(normalize=False), storage="ivfpq", codec=codec)
    with pytest.raises(ValueError, match=r"storage='ivfpq' holds single \(\[CLS\]\) vectors only"):
        tok.add(docs)
    narrow = CorpusIndex(TableModel(c["table"], torch.float32, False), InBatchDotScores(), storage="ivfpq",
                         codec=IVFPQCodec(p["cent"][:, :16], p["cb"][:4]))
    with pytest.raises(ValueError, match="quantises vectors of 16 features"):
        narrow.add(docs)
    index = CorpusIndex(TableModel(c["table"], torch.float32, False), InBatchDotScores(), storage="ivfpq", codec=codec)
    index.add(docs)
    for call in (lambda: index.rerank(queries, np.zeros((5, 1), np.int64), 1), lambda: index.fit_centroids(4),
                 lambda: index.set_centroids(np.zeros((4, 32), np.float32)), lambda: index.search_pruned(queries, 3, 10),
                 lambda: index.search_pruned(queries, 3, 10, nprobe=2), lambda: index.probe(queries, 2)):
        with pytest.raises(ValueError, match=r"\[CLS\]"):
            call()
    for call in (lambda: index.fit_pq(8, 16), lambda: index.fit_ivfpq(4, 8, 16)):
        with pytest.raises(ValueError, match="plain \\[CLS\\] index"):
            call()
    for bad in (0, K + 1):
        with pytest.raises(ValueError, match=rf"need 1 <= nprobe <= min\(K, 1024\) = {K}"):
            index.search(queries, 3, nprobe=bad)
    plain = CorpusIndex(TableModel(c["table"], torch.float32, False), InBatchDotScores())
    plain.add(docs)
    with pytest.raises(ValueError, match="nprobe belongs to storage='ivfpq'"):
        plain.search(queries, 3, nprobe=2)
    with pytest.raises(ValueError, match=r"max\(K, ksub\) = 41"):
        plain.fit_ivfpq(41, 8, 16)
    with pytest.raises(ValueError, match="must divide"):
        plain.fit_ivfpq(4, 12, 16)
    val, idx = _np(index.search(queries, 100))                 # fewer than k documents: the tail is (-inf, -1)
    assert (idx[:, 40:] == -1).all() and (val[:, 40:] == -np.inf).all() and (idx[:, :40] >= 0).all()
    val1, idx1 = _np(index.search(queries, 100, nprobe=1))     # fewer than k candidates: the same padding
    sizes = np.bincount(p["coarse"][:40], minlength=K)
    cdot = (p["q"].astype(np.float64) @ p["cent"].astype(np.float64).T).astype(np.float32)
    for b in range(len(p["q"])):
        n = int(sizes[ir.probes(cdot, 1)[b, 0]])
        assert (idx1[b, :n] >= 0).all() and (idx1[b, n:] == -1).all() and (val1[b, n:] == -np.inf).all()
        assert (p["coarse"][idx1[b, :n]] == ir.probes(cdot, 1)[b, 0]).all()
    assert index.lists is not None and index.nbytes == 40 * (m + 2) + 4 * (K + 1) + 4 * 40
    index.clear()
    assert len(index) == 0 and index.pq_codes is None and index.coarse_codes is None and index.lists is None
    assert index.codec is codec and index.nbytes == 0 and index.centroids is codec.centroids
    index.add(docs)                                            # a cleared index takes documents again
    assert len(index) == 40 and np.array_equal(index.coarse_codes.cpu().numpy().view(np.uint16), p["coarse"][:40])
