"""CorpusIndex with centroids on the device (TableModel stand-ins, f32 and bf16, plain and FP8 storage): lossless
centroids, equality with the exhaustive search when every document is a candidate, chunking, incremental adds, the
k-means fit on a planted corpus, the refusals, and the validation callback."""
import numpy as np
import pytest
import torch

from tests import centroid_ref as cr, search_ref as sr
from tests.centroid_cases import planted_corpus
from tests.search_cases import TableModel, batches, cls_case, maxsim_tol, token_case
from tests.util import host

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
CASE = dict(seed=21, Q=8, N=300, Lq=8, Ld=16, E=64, V=256)
STORAGES = [None, "fp8"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _index(c, mode, storage=None, sizes=None, **kw):
    from polus_amd.ir.search import CorpusIndex
    from polus_amd.ir.training import MaxSimScores
    index = CorpusIndex(TableModel(c["table"], DT[mode], True), MaxSimScores(normalize=True), storage=storage, **kw)
    n = len(c["d_ids"])
    for b in batches(c["d_ids"], c["d_mask"], sizes or [n // 2, n - n // 2]):
        index.add(b)
    return index, {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}


def _same(got, want, what):
    got, want = [t.cpu().numpy() for t in got], [t.cpu().numpy() for t in want]
    assert np.array_equal(got[1], want[1]), f"{what}: ids differ in {int((got[1] != want[1]).sum())} places"
    assert np.array_equal(_bits(got[0]), _bits(want[0])), f"{what}: values differ"


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_lossless_centroids(mode, storage):
    """256 distinct table rows, the centroids those rows normalised in the index's dtype: a token's nearest centroid is
    its own row, so the codes are the token ids (plain index) and the look-up score is the MaxSim score up to rounding."""
    from polus_amd import ops
    c = token_case(**CASE)
    index, queries = _index(c, mode, storage)
    t = torch.as_tensor(c["table"]).to(DT[mode]).cuda()
    cent, rn = torch.empty_like(t), torch.empty((len(t),), dtype=torch.float32, device="cuda")
    ops.l2norm_fwd(t, cent, rn)
    before = index.nbytes
    index.set_centroids(cent)
    assert torch.equal(index.centroids, cent) and index.centroids.data_ptr() != cent.data_ptr()
    codes = index.centroid_codes
    assert codes.dtype == torch.int16 and tuple(codes.shape) == (CASE["N"], CASE["Ld"])
    assert index.nbytes == before + 2 * CASE["N"] * CASE["Ld"]
    got = codes.cpu().numpy().view(np.uint16)
    assert (got[c["d_mask"] == 0] == 0xFFFF).all()
    if storage is None:
        assert np.array_equal(got[c["d_mask"] != 0], c["d_ids"][c["d_mask"] != 0].astype(np.uint16))
    q = index.encode_queries(queries)
    s64 = sr.maxsim_scores(host(q.values), host(index.representations), c["q_mask"], c["d_mask"])
    tol = maxsim_tol(mode) * np.abs(s64).max()
    val, idx = index.search_pruned(queries, 10, 40)
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and tuple(idx.shape) == (CASE["Q"], 10)
    assert sr.check_against_float64(val.cpu().numpy(), idx.cpu().numpy(), s64, 10, tol) == []


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_every_document_a_candidate_gives_the_bits_of_search(mode, storage):
    """candidates >= len(index): the approximate stage cannot matter, so this pins the plumbing (one query encoding,
    the candidate ids, the rerank path).  Also with several chunks of documents and of candidates."""
    c = token_case(**CASE)
    index, queries = _index(c, mode, storage)
    index.fit_centroids(8)
    assert tuple(index.centroids.shape) == (8, CASE["E"]) and index.centroids.dtype == DT[mode]
    for k in (10, 400):                                                # 400 > N: padded with (-inf, -1)
        want = index.search(queries, k)
        _same(index.search_pruned(queries, k, 1024), want, f"{mode} {storage} k={k}")
        _same(index.search_pruned(queries, k, CASE["N"]), want, f"{mode} {storage} k={k} candidates=N")
    big = index.scratch_bytes
    index.scratch_bytes = 4 * CASE["Q"] * 70
    assert len(index.chunks(CASE["Q"])) == 5 and len(index.rerank_chunks(CASE["Q"], CASE["N"])) == 5
    _same(index.search_pruned(queries, 10, CASE["N"]), want := index.search(queries, 10), "chunked")
    index.scratch_bytes = big
    _same(index.search_pruned(queries, 10, CASE["N"]), want, "unchunked")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_chunking_does_not_change_the_result(mode):
    c = token_case(**CASE)
    index, queries = _index(c, mode)
    index.fit_centroids(32, iters=2)
    want = index.search_pruned(queries, 10, 40)
    cv, ci = want[0].cpu().numpy(), want[1].cpu().numpy()
    assert (ci >= 0).all() and np.isfinite(cv).all()
    index.scratch_bytes = 4 * CASE["Q"] * 25                           # 12 chunks of documents, 2 of candidates
    assert len(index.chunks(CASE["Q"])) == 12 and len(index.rerank_chunks(CASE["Q"], 40)) == 2
    _same(index.search_pruned(queries, 10, 40), want, f"{mode} chunked")
    # every returned score is the exact MaxSim score of its document: the bits `search` gives it
    full = index.search(queries, CASE["N"])
    fv, fi = full[0].cpu().numpy(), full[1].cpu().numpy()
    for r in range(CASE["Q"]):
        exact = dict(zip(fi[r].tolist(), _bits(fv[r]).tolist()))
        assert [exact[i] for i in ci[r].tolist()] == _bits(cv[r]).tolist()


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_documents_added_after_the_fit_get_the_codes_of_a_full_assignment(mode, storage):
    from polus_amd.ir.search import CorpusIndex
    from polus_amd.ir.training import MaxSimScores
    c = token_case(**CASE)
    index = CorpusIndex(TableModel(c["table"], DT[mode], True), MaxSimScores(normalize=True), storage=storage)
    parts = batches(c["d_ids"], c["d_mask"], [120, 1, 179], [16, 9, 16])
    index.add(parts[0])
    index.fit_centroids(16, iters=2, seed=3)
    cent = index.centroids.clone()
    first = index.centroid_codes.clone()
    index.add(parts[1])                                                # grows the buffers: the codes are carried over
    index.add(parts[2])
    assert torch.equal(index.centroids, cent) and torch.equal(index.centroid_codes[:120], first)
    codes = index.centroid_codes.clone()
    assert tuple(codes.shape) == (300, 16)
    got = codes.cpu().numpy().view(np.uint16)
    mask = index.mask.cpu().numpy()
    assert (got[mask == 0] == 0xFFFF).all() and (got[mask != 0] < 16).all() and (got[120, 9:] == 0xFFFF).all()
    index.set_centroids(index.centroids)
    assert torch.equal(index.centroid_codes, codes)
    index.clear()
    assert index.centroids is None and index.centroid_codes is None and index.nbytes == 0


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_fit_on_a_planted_corpus(mode):
    """24 unit directions in E = 32, 3000 tokens = direction + 0.35 N(0, I) / sqrt(E) renormalised, K = 16: three rounds
    raise the mean best similarity by more than 0.1 (the NumPy algorithm: 0.51-0.66 -> 0.79-0.82 over six seeds; bf16
    rounding moves it by at most 2^-8), every centroid has unit norm within the dtype's rounding, the same seed gives
    the same bits and another seed other centroids."""
    x = planted_corpus()
    c = dict(table=x, d_ids=np.arange(3000, dtype=np.int32).reshape(300, 10), d_mask=np.ones((300, 10), np.int32),
             q_ids=np.zeros((1, 1), np.int32), q_mask=np.ones((1, 1), np.int32))
    index, _ = _index(c, mode)
    tokens = host(index.representations).reshape(3000, 32)
    best = {}
    for iters in (0, 3):
        index.fit_centroids(16, iters=iters, seed=5)
        cent = host(index.centroids)
        best[iters] = cr.mean_best_similarity(tokens, cent)
        unit = 2.0 ** -8 if mode == "bf16" else 32 * 2.0 ** -24
        assert np.abs(np.linalg.norm(cent, axis=1) - 1).max() <= unit, iters
        codes = index.centroid_codes.cpu().numpy().view(np.uint16)
        assert codes.max() < 16 and len(np.unique(codes)) > 8
    print(f"{mode}: mean best similarity {best[0]:.3f} -> {best[3]:.3f}")
    assert best[3] - best[0] > 0.1
    first = index.centroids.clone()
    index.fit_centroids(16, iters=3, seed=5)
    assert torch.equal(index.centroids, first), "the same seed gave other bits"
    index.fit_centroids(16, iters=3, seed=6)
    assert not torch.equal(index.centroids, first), "another seed gave the same centroids"
    index.fit_centroids(16, iters=3, seed=5, sample=1000)              # a true sample: 1000 of the 3000 slots
    assert cr.mean_best_similarity(tokens, host(index.centroids)) - best[0] > 0.1


def test_refusals():
    from polus_amd.ir.search import CorpusIndex
    from polus_amd.ir.training import InBatchDotScores, MaxSimScores
    c = token_case(2, 4, 20, 4, 8, 32, 64)
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    docs = {"input_ids": c["d_ids"], "attention_mask": c["d_mask"]}
    valid = int((c["d_mask"] != 0).sum())
    cc = cls_case(2, 4, 20, 32)
    cls_index = CorpusIndex(TableModel(cc["table"], torch.float32, False), InBatchDotScores())
    cls_index.add({"input_ids": cc["d_ids"], "attention_mask": cc["d_mask"]})
    with pytest.raises(ValueError, match=r"\[CLS\]"):
        cls_index.fit_centroids(4)
    plain = CorpusIndex(TableModel(c["table"], torch.float32, True), MaxSimScores(normalize=False))
    plain.add(docs)
    with pytest.raises(ValueError, match="normalize=True"):
        plain.fit_centroids(4)
    index = CorpusIndex(TableModel(c["table"], torch.float32, True), MaxSimScores(normalize=True))
    for call in (lambda: index.fit_centroids(4), lambda: index.search_pruned(queries, 3, 10)):
        with pytest.raises(ValueError, match="empty"):
            call()
    index.add(docs)
    with pytest.raises(ValueError, match="needs centroids"):
        index.search_pruned(queries, 3, 10)
    with pytest.raises(ValueError, match="valid sampled tokens"):
        index.fit_centroids(valid + 1)
    with pytest.raises(ValueError, match="valid sampled tokens"):
        index.fit_centroids(60, sample=50)
    with pytest.raises(ValueError, match="65535"):
        index.fit_centroids(65536)
    with pytest.raises(ValueError, match="65535"):
        index.set_centroids(np.zeros((65536, 32), np.float32))
    with pytest.raises(ValueError, match=r"\[K, 32\]"):
        index.set_centroids(np.zeros((4, 16), np.float32))
    assert index.centroids is None
    index.fit_centroids(valid)                                         # as many centroids as valid tokens is allowed
    with pytest.raises(ValueError, match="limit of ops.topk_merge"):
        index.search_pruned(queries, 3, 1025)
    val, idx = index.search_pruned(queries, 3, 1024)
    assert tuple(idx.shape) == (4, 3) and (idx.cpu().numpy() >= 0).all()


def test_validation_callback_with_centroids_matches_the_exhaustive_one():
    """As tests/test_search_gpu.py drives the callback: a tiny BERT, one epoch, two callbacks over the same corpus and
    validation data, one exhaustive and one with centroids and every document a candidate: the same metrics."""
    from polus_amd.ir.metrics import MRRAtK, NDCGAtK, RecallAtK
    from polus_amd.ir.models import LateInteractionDualEncoder
    from polus_amd.ir.search import RetrievalValidationCallback
    from polus_amd.ir.training import ContrastiveLoss, EfficientDenseRetrievalTrainer, MaxSimScores
    from polus_amd.models import BertConfig, BertModel
    from polus_amd.optimizers import Adam
    from tests.test_model_gpu import load_case
    _, ocfg, params, _, _ = load_case("bert_small_b3_s48")
    cfg = BertConfig(ocfg.vocab_size, ocfg.hidden_size, ocfg.num_hidden_layers, ocfg.num_attention_heads,
                     ocfg.intermediate_size, ocfg.max_position_embeddings, ocfg.type_vocab_size)
    enc = BertModel(cfg, compute_dtype="bf16"); enc.load_numpy_params(params)
    r = np.random.Generator(np.random.PCG64(43))

    def batch(n, S):
        lens = r.integers(2, S + 1, size=n)
        return {"input_ids": r.integers(1, ocfg.vocab_size, size=(n, S)).astype(np.int32),
                "attention_mask": (np.arange(S) < lens[:, None]).astype(np.int32)}
    B, Sq, Sd, E, K = 6, 12, 40, 64, 5
    model, scorer = LateInteractionDualEncoder(enc, projection_dim=E, compute_dtype="bf16"), MaxSimScores(normalize=True)
    train = [(batch(B, Sq), batch(B, Sd)) for _ in range(2)]
    corpus = [batch(7, Sd), batch(5, Sd - 16)]
    relevant = [set(range(8)), {0, 11}, {3: 2.0, 9: 1.0}, [5, 6, 7, 8, 9, 10, 11, 0]]
    val = [(batch(2, Sq), relevant[:2]), (batch(2, Sq), relevant[2:])]
    metrics = [RecallAtK(K), MRRAtK(K), NDCGAtK(K)]
    trainer = EfficientDenseRetrievalTrainer(model, scorer, optimizer=Adam(1e-3), loss=ContrastiveLoss(), metrics=metrics)
    pruned = RetrievalValidationCallback(corpus, val, K, name="pruned", centroids=8, candidates=12)
    assert pruned.candidates == 12 and RetrievalValidationCallback(corpus, val, K, centroids=8).candidates == 1024
    trainer.train(train, epochs=1, callbacks=[RetrievalValidationCallback(corpus, val, K, name="full"), pruned])
    torch.cuda.synchronize()
    res = trainer.callbacks.shared_dict["validation"]
    assert sorted(res["pruned"]) == sorted(m.name for m in metrics)
    for name in res["full"]:
        assert res["pruned"][name] == res["full"][name] and len(res["full"][name]) == 1, name
    assert res["full"][f"Recall@{K}"][0] > 0
