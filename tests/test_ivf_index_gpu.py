"""CorpusIndex.search_pruned(..., nprobe) on the device (TableModel stand-ins, f32 and bf16, plain, FP8 and residual
storage): every centroid probed gives the bits of the scan, few probes give exactly the reference's candidates for the
device's own probes, the probes are the nearest centroids, empty documents, stale lists, nbytes, the refusals and the
validation callback."""
import numpy as np
import pytest
import torch

from tests import ivf_ref as ir
from tests.search_cases import TableModel, batches, cls_case, maxsim_tol, token_case
from tests.util import host

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
CASE = dict(seed=21, Q=8, N=300, Lq=8, Ld=16, E=64, V=256)
STORAGES = [None, "fp8", "residual"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _plain(c, mode, storage=None, sizes=None, **kw):
    from polus_amd.ir.search import CorpusIndex
    from polus_amd.ir.training import MaxSimScores
    index = CorpusIndex(TableModel(c["table"], DT[mode], True), MaxSimScores(normalize=True), storage=storage, **kw)
    n = len(c["d_ids"])
    for b in batches(c["d_ids"], c["d_mask"], sizes or [n // 2, n - n // 2]):
        index.add(b)
    return index


def _index(c, mode, storage, K):
    """An index of the case's documents with K fitted centroids; a residual index takes them, as a codec, from a plain
    index fitted the same way."""
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    if storage == "residual":
        trainer = _plain(c, mode)
        trainer.fit_centroids(K)
        return _plain(c, mode, "residual", codec=trainer.fit_codec(2)), queries
    index = _plain(c, mode, storage)
    index.fit_centroids(K)
    return index, queries


def _same(got, want, what):
    got, want = [t.cpu().numpy() for t in got], [t.cpu().numpy() for t in want]
    assert np.array_equal(got[1], want[1]), f"{what}: ids differ in {int((got[1] != want[1]).sum())} places"
    assert np.array_equal(_bits(got[0]), _bits(want[0])), f"{what}: values differ"


def _full_case():
    c = token_case(**CASE)
    c["d_mask"][1, 0] = 1                                              # every document has a present token
    return c


def _host_lists(index):
    offsets, docs = index.lists
    return ir.split(offsets.cpu().numpy(), docs.cpu().numpy())


def _codes(index):
    return index.centroid_codes.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_every_centroid_probed_gives_the_bits_of_the_scan(mode, storage):
    c = _full_case()
    N, Q = CASE["N"], CASE["Q"]
    index, queries = _index(c, mode, storage, 8)
    for k, cands in ((10, 40), (10, N), (400, 1024)):
        _same(index.search_pruned(queries, k, cands, nprobe=8), index.search_pruned(queries, k, cands),
              f"{mode} {storage} k={k} candidates={cands}")
    # 64 centroids and a scratch of 2240 bytes: one query per probe GEMM (2048 bytes of similarities each), one query per
    # candidate buffer (300 ids = 1200 bytes), five chunks of documents in the scan and of candidates in the rerank
    index, queries = _index(c, mode, storage, 64)
    want = [index.search_pruned(queries, k, cands) for k, cands in ((10, 40), (400, 1024))]
    index.scratch_bytes = 4 * Q * 70
    assert len(index.chunks(Q)) == 5 and len(index.rerank_chunks(Q, N)) == 5
    assert index.scratch_bytes // (4 * CASE["Lq"] * 64) == 1 and 2 * 4 * N > index.scratch_bytes
    _same(index.search_pruned(queries, 10, 40, nprobe=64), want[0], f"{mode} {storage} chunked")
    _same(index.search_pruned(queries, 400, 1024, nprobe=64), want[1], f"{mode} {storage} chunked k=400")
    _, _, count = index.probe(queries, 64)
    assert count.cpu().tolist() == [N] * Q


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_few_probes_give_the_reference_candidates_of_the_device_probes(mode, storage):
    c = token_case(**CASE)
    N, Q, Lq = CASE["N"], CASE["Q"], CASE["Lq"]
    for K in (8, 64):
        index, queries = _index(c, mode, storage, K)
        per_centroid = _host_lists(index)
        assert per_centroid == ir.lists(_codes(index), K)[2]
        q = index.encode_queries(queries)
        sim = host(q.values) @ host(index.centroids).T                  # float64 [Q, Lq, K] of what the device holds
        tol = maxsim_tol(mode) * np.abs(sim).max()
        for nprobe in (1, 2):
            probes, cand, count = index.probe(queries, nprobe)
            assert probes.dtype == torch.int32 and tuple(probes.shape) == (Q, Lq, nprobe)
            assert cand.dtype == torch.int32 and count.dtype == torch.int32 and tuple(count.shape) == (Q,)
            p, ch, cn = probes.cpu().numpy(), cand.cpu().numpy(), count.cpu().numpy()
            assert ((p >= 0) & (p < K)).all() and ch.shape == (Q, max(1, cn.max()))
            want = ir.candidates(p, c["q_mask"], per_centroid, N)
            for b in range(Q):
                assert cn[b] == len(want[b]) and ch[b, :cn[b]].tolist() == sorted(want[b]) and (ch[b, cn[b]:] == -1).all()
            assert 1 not in set(ch.reshape(-1).tolist())               # document 1 holds no token
            kth = -np.sort(-sim, axis=2)[:, :, nprobe - 1]
            got = np.take_along_axis(sim, p.astype(np.int64), axis=2)
            worst = float((kth[:, :, None] - got).max())
            print(f"{mode} {storage} K={K} nprobe={nprobe}: candidates {cn.min()}..{cn.max()}, worst shortfall {worst:.3e} (tol {tol:.3e})")
            assert (got >= kth[:, :, None] - tol).all()
            if nprobe == 2:
                assert (p[:, :, 0] != p[:, :, 1]).all()
            _same(index.search_pruned(queries, 10, 1024, nprobe=nprobe), index.rerank(queries, cand, 10),
                  f"{mode} {storage} K={K} nprobe={nprobe}")
        if K == 64:
            assert cn.max() < N                                            # two probes of 64 do not reach every document


@pytest.mark.parametrize("storage", STORAGES)
def test_a_document_without_tokens_is_never_a_candidate(storage):
    c = token_case(**CASE)
    N = CASE["N"]
    index, queries = _index(c, "f32", storage, 8)
    val, ids = [t.cpu().numpy() for t in index.search_pruned(queries, 400, 1024, nprobe=8)]
    sv, si = [t.cpu().numpy() for t in index.search_pruned(queries, 400, 1024)]
    assert (si[:, :N] >= 0).all() and (si == 1).sum() == CASE["Q"]     # the scan ranks it (score 0.0)
    for r in range(CASE["Q"]):
        assert 1 not in ids[r].tolist()
        assert (ids[r, N - 1:] == -1).all() and np.isneginf(val[r, N - 1:]).all()
        keep = si[r, :N] != 1
        assert ids[r, :N - 1].tolist() == si[r, :N][keep].tolist()
        assert _bits(val[r, :N - 1]).tolist() == _bits(sv[r, :N][keep]).tolist()


def test_lists_follow_add_set_centroids_and_clear():
    from polus_amd.ir.search import CorpusIndex
    from polus_amd.ir.training import MaxSimScores
    c = _full_case()
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    index = CorpusIndex(TableModel(c["table"], torch.float32, True), MaxSimScores(normalize=True))
    parts = batches(c["d_ids"], c["d_mask"], [120, 1, 179], [16, 9, 16])
    index.add(parts[0])
    assert index.lists is None                                         # no centroids yet
    index.fit_centroids(16, iters=2, seed=3)
    before = index.nbytes
    index.search_pruned(queries, 10, 40)
    assert index.nbytes == before                                      # the scan builds nothing
    ids = index.search_pruned(queries, 400, 1024, nprobe=16)[1].cpu().numpy()
    assert ids.max() == 119 and (np.sort(ids[:, :120], axis=1) == np.arange(120)).all()
    offsets, docs = index.lists
    P = int(offsets[-1])
    assert tuple(offsets.shape) == (17,) and tuple(docs.shape) == (P,) and index.nbytes == before + 4 * 17 + 4 * P
    index.add(parts[1])
    index.add(parts[2])
    ids = index.search_pruned(queries, 400, 1024, nprobe=16)[1].cpu().numpy()
    assert (np.sort(ids[:, :300], axis=1) == np.arange(300)).all()      # the new documents are reachable
    _same(index.search_pruned(queries, 10, 40, nprobe=16), index.search_pruned(queries, 10, 40), "after add")
    assert _host_lists(index) == ir.lists(_codes(index), 16)[2]
    other = index.representations[5:300:37, 0].contiguous()            # 8 stored token vectors as centroids
    index.set_centroids(other)
    lists = _host_lists(index)
    assert len(lists) == 8 and lists == ir.lists(_codes(index), 8)[2]
    _same(index.search_pruned(queries, 10, 40, nprobe=8), index.search_pruned(queries, 10, 40), "after set_centroids")
    index.clear()
    assert index.lists is None and index.nbytes == 0


def test_refusals_and_the_probe_limit():
    from polus_amd.ir.search import CorpusIndex, RetrievalValidationCallback
    from polus_amd.ir.training import InBatchDotScores, MaxSimScores
    c = token_case(**CASE)
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    cc = cls_case(2, 4, 20, 32)
    cls_index = CorpusIndex(TableModel(cc["table"], torch.float32, False), InBatchDotScores())
    cls_index.add({"input_ids": cc["d_ids"], "attention_mask": cc["d_mask"]})
    cls_queries = {"input_ids": cc["q_ids"], "attention_mask": cc["q_mask"]}
    with pytest.raises(ValueError, match=r"\[CLS\]"):
        cls_index.fit_centroids(4)
    for call in (lambda: cls_index.search_pruned(cls_queries, 3, 10, nprobe=1), lambda: cls_index.probe(cls_queries, 1),
                 lambda: cls_index.refresh_lists()):
        with pytest.raises(ValueError, match="needs centroids"):
            call()
    index = _plain(c, "f32")
    for call in (lambda: index.search_pruned(queries, 3, 10, nprobe=1), lambda: index.probe(queries, 1)):
        with pytest.raises(ValueError, match="needs centroids"):
            call()
    index.fit_centroids(8)
    for bad in (0, -1, 9):
        with pytest.raises(ValueError, match=r"1 <= nprobe <= min\(K, 1024\) = 8"):
            index.search_pruned(queries, 3, 10, nprobe=bad)
        with pytest.raises(ValueError, match=r"1 <= nprobe <= min\(K, 1024\) = 8"):
            index.probe(queries, bad)
    assert index.nbytes == 300 * 16 * (64 * 4 + 4 + 2)                 # none of the refused calls built the lists
    with pytest.raises(ValueError, match="nprobe needs centroids"):
        RetrievalValidationCallback([], [], 5, nprobe=2)
    with pytest.raises(ValueError, match="nprobe >= 1"):
        RetrievalValidationCallback([], [], 5, centroids=8, nprobe=0)
    # more centroids than ops.topk_merge keeps: 1024 probes per token is the most, and runs (32 tiles of probes per query)
    r = np.random.Generator(np.random.PCG64(77))
    index.set_centroids(r.standard_normal((1100, CASE["E"])).astype(np.float32))
    with pytest.raises(ValueError, match=r"= 1024"):
        index.search_pruned(queries, 3, 10, nprobe=1025)
    probes, cand, count = index.probe(queries, 1024)
    want = ir.candidates(probes.cpu().numpy(), c["q_mask"], _host_lists(index), CASE["N"])
    ch, cn = cand.cpu().numpy(), count.cpu().numpy()
    for b in range(CASE["Q"]):
        assert ch[b, :cn[b]].tolist() == sorted(want[b])


def test_validation_callback_with_nprobe_matches_the_scan():
    """As tests/test_centroid_index_gpu.py drives the callback: a tiny BERT, one epoch, two callbacks over the same corpus
    and validation data with the same centroids and candidates, one scanning and one probing every centroid: the same
    metrics (every document of the corpus has a valid token)."""
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
    probed = RetrievalValidationCallback(corpus, val, K, name="probed", centroids=8, candidates=6, nprobe=8)
    scan = RetrievalValidationCallback(corpus, val, K, name="scan", centroids=8, candidates=6)
    assert probed.nprobe == 8 and scan.nprobe is None
    trainer.train(train, epochs=1, callbacks=[scan, probed])
    torch.cuda.synchronize()
    res = trainer.callbacks.shared_dict["validation"]
    assert sorted(res["probed"]) == sorted(m.name for m in metrics)
    for name in res["scan"]:
        assert res["probed"][name] == res["scan"][name] and len(res["scan"][name]) == 1, name
    assert res["scan"][f"Recall@{K}"][0] > 0
