"""Corpus search on the device against the NumPy reference of tests/search_ref.py: polus_topk_merge (exact ids and
values over shapes, ties, special values, strides, chunkings, guards), polus_maxsim_scores (bitwise the scores of
polus_maxsim_fwd), CorpusIndex.search (exact on integer data, identical to the reference selection over the same
launches, within the kernels' measured tolerance of float64), normalised MaxSim on a planted corpus, the validation
callback end to end on a tiny BERT, and the refusals."""
import numpy as np
import pytest
import torch

from tests import maxsim_ref, search_ref as sr
from tests.maxsim_cases import MASKS, SHAPES, TOL, make_case
from tests.search_cases import (CLS_CASE, KS, TOKEN_CASE, TableEncoder, TableModel, batches, cls_case, dot_tol,
                                maxsim_tol, token_case)
from tests.util import assert_close, host, rounded

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
GUARD = 64


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _merge(scores, k, id0=0, lds=None, col0=0, state=None, garbage=False):
    """One polus_topk_merge call over a host array: the scores sit at columns col0 .. col0+n of a [rows, lds] buffer
    whose other columns hold 3e38; the state buffers carry GUARD elements behind [rows, k], which must stay as they
    were.  state = (vals, ids) continues a merge, None starts one (garbage: over a state full of NaN and wild ids)."""
    from polus_amd import ops
    rows, n = scores.shape
    lds = lds or (col0 + n)
    buf = torch.full((rows, lds), 3e38, dtype=torch.float32, device="cuda")
    buf[:, col0:col0 + n] = torch.as_tensor(scores)
    tv = torch.full((rows * k + GUARD,), 777.0, dtype=torch.float32, device="cuda")
    ti = torch.full((rows * k + GUARD,), 424242, dtype=torch.int32, device="cuda")
    if state is not None:
        tv[:rows * k] = torch.as_tensor(state[0]).reshape(-1)
        ti[:rows * k] = torch.as_tensor(state[1]).reshape(-1)
    elif garbage:
        tv[:rows * k] = float("nan")
        ti[:rows * k:2] = 2 ** 31 - 1
    ops.topk_merge(buf[:, col0:col0 + n], tv[:rows * k].view(rows, k), ti[:rows * k].view(rows, k), id0=id0,
                   init=state is None)
    torch.cuda.synchronize()
    assert (tv[rows * k:] == 777.0).all() and (ti[rows * k:] == 424242).all(), "guard elements were written"
    return tv[:rows * k].view(rows, k).cpu().numpy(), ti[:rows * k].view(rows, k).cpu().numpy()


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), f"{what}: ids differ in {int((got[1] != want[1]).sum())} places"
    assert np.array_equal(_bits(got[0]), _bits(want[0])), f"{what}: values differ"


def _draw(kind, r, rows, n):
    if kind == "normal":
        return r.standard_normal((rows, n)).astype(np.float32)
    if kind == "ties":
        return r.choice(np.array([-1.5, 0.25, 0.25000003, 7.0], np.float32), size=(rows, n))
    s = r.standard_normal((rows, n)).astype(np.float32)                # "special"
    u = r.random((rows, n))
    for lo, hi, v in ((0.00, 0.05, np.nan), (0.05, 0.10, -np.inf), (0.10, 0.13, np.inf), (0.13, 0.18, 0.0), (0.18, 0.23, -0.0)):
        s[(u >= lo) & (u < hi)] = v
    s[rows - 1] = -np.inf                                              # a row that returns only padding
    return s


@pytest.mark.parametrize("kind", ["normal", "ties", "special"])
def test_topk_merge_matches_reference_exactly(kind):
    r = np.random.Generator(np.random.PCG64({"normal": 1, "ties": 2, "special": 3}[kind]))
    for rows in (1, 3, 64):
        for n in (1, 7, 64, 1000, 65535):
            s = _draw(kind, r, rows, n)
            id0 = int(r.integers(0, 1000)) if n != 7 else 2 ** 31 - 1 - n     # id0 > 0, once up against the limit
            full = sr.topk(s, 1024, id0=id0)                                # a prefix of it is the answer for k < 1024
            for k in (1, 10, 100, 1024):
                # odd row strides and a column offset: rows start at every 4-byte phase of a 16-byte line
                got = _merge(s, k, id0=id0, lds=n + 7, col0=int(r.integers(0, 4)))
                _same(got, (full[0][:, :k], full[1][:, :k]), f"{kind} rows={rows} n={n} k={k}")
                if kind == "special":
                    assert (got[1][rows - 1] == -1).all() and np.isneginf(got[0][rows - 1]).all()


def test_topk_merge_chunkings_repeat_runs_and_garbage_state():
    r = np.random.Generator(np.random.PCG64(11))
    rows, n = 3, 20000
    for kind, k in (("normal", 100), ("ties", 1024), ("special", 10), ("normal", 1024)):
        s = _draw(kind, r, rows, n)
        want = sr.topk(s, k)
        once = _merge(s, k)
        _same(once, want, f"{kind} single call")
        _same(_merge(s, k), once, f"{kind} second run")
        _same(_merge(s, k, garbage=True), once, f"{kind} init over a garbage state")
        for trial in range(3):
            cuts = np.unique(np.concatenate([[0, n], r.integers(1, n, size=int(r.integers(1, 9)))]))
            state = None
            for a, b in zip(cuts[:-1], cuts[1:]):
                state = _merge(s[:, a:b], k, id0=int(a), state=state)
            _same(state, once, f"{kind} k={k} cuts={cuts.tolist()}")
    # ascending scores: every column beats the threshold, the buffer fills and is sorted over and over
    s = np.sort(r.standard_normal((2, 65535)).astype(np.float32), axis=1)
    for k in (100, 1024):
        _same(_merge(s, k), sr.topk(s, k), f"ascending k={k}")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_maxsim_scores_equal_maxsim_fwd_bitwise(mode):
    from polus_amd import ops
    for shape in SHAPES:
        for masks in MASKS:
            q, d, qm, dm = make_case(shape, masks)
            B, N, Lq = q.shape[0], d.shape[0], q.shape[1]
            dev = lambda a, dt=None: None if a is None else (torch.as_tensor(np.ascontiguousarray(a)).to(dt) if dt else torch.as_tensor(np.ascontiguousarray(a))).cuda()
            qt, dt_, qmt, dmt = dev(q, DT[mode]), dev(d, DT[mode]), dev(qm), dev(dm)
            s_fwd = torch.full((B, N), float("nan"), dtype=torch.float32, device="cuda")
            am = torch.empty((B, N, Lq), dtype=torch.int32, device="cuda")
            ops.maxsim_fwd(qt, dt_, qmt, dmt, s_fwd, am)
            s = torch.full((B, N), float("nan"), dtype=torch.float32, device="cuda")
            ops.maxsim_scores(qt, dt_, qmt, dmt, s)
            wide = torch.full((B, 2 * N + 3), -7.25, dtype=torch.float32, device="cuda")
            ops.maxsim_scores(qt, dt_, qmt, dmt, wide[:, 1:1 + N])
            torch.cuda.synchronize()
            assert torch.equal(s.view(torch.int32), s_fwd.view(torch.int32)), (shape, masks)
            assert torch.equal(wide[:, 1:1 + N].contiguous().view(torch.int32), s_fwd.view(torch.int32)), (shape, masks)
            assert (wide[:, 0] == -7.25).all() and (wide[:, 1 + N:] == -7.25).all()


def _int_weights(model, seed):
    r = np.random.Generator(np.random.PCG64(seed))
    ws = []
    for v in model.trainable_weights:
        w = r.integers(-1, 2, size=v.shape).astype(np.float32) if len(v.shape) == 2 else np.zeros(v.shape, np.float32)
        v.assign(w)
        ws.append(w.astype(np.float64))
    return ws                                                          # query W, b, document W, b


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["tokens", "cls"])
def test_corpus_index_exact_on_integer_data(kind, mode):
    """Integer encoder states in [-2, 2] (or [-3, 3]) and projection weights in {-1, 0, 1}, H = E = 32: projections
    (|p| <= 96), products and sums (< 2^24) are exact in bf16 and f32, so ids and scores equal the float64 ranking
    bit for bit, ties included.  Four `add` calls of unequal sizes and lengths, three chunks, an empty document."""
    from polus_amd.ir.models import DualEncoder, LateInteractionDualEncoder
    from polus_amd.ir.search import CorpusIndex
    from polus_amd.ir.training import InBatchDotScores, MaxSimScores
    Q, N, sizes = 12, 700, [300, 1, 250, 149]
    if kind == "tokens":
        c = token_case(5, Q, N, Lq=8, Ld=24, E=32, V=512, integer=True)
        lengths = [24, 10, 17, 24]
        model = LateInteractionDualEncoder(TableEncoder(c["table"]), projection_dim=32, compute_dtype=mode)
        scorer = MaxSimScores(normalize=False)
    else:
        c = cls_case(5, Q, N, E=32, integer=True)
        lengths = None
        model = DualEncoder(TableEncoder(c["table"]), projection_dim=32, compute_dtype=mode)
        scorer = InBatchDotScores()
    wq, _, wd, _ = _int_weights(model, 6)
    index = CorpusIndex(model, scorer, scratch_bytes=4 * Q * 260)
    ids = [index.add(b) for b in batches(c["d_ids"], c["d_mask"], sizes, lengths)]
    assert torch.equal(torch.cat(ids).cpu(), torch.arange(N, dtype=torch.int32)) and len(index) == N
    assert index.chunks(Q) == [(0, 260), (260, 520), (520, 700)]
    assert index.representations.is_contiguous() and index.representations.dtype == DT[mode]
    tab = c["table"].astype(np.float64)
    pq, pd_ = tab[c["q_ids"]] @ wq.T, tab[c["d_ids"]] @ wd.T
    if kind == "tokens":
        dm = c["d_mask"].copy()
        a = 0
        for n, L in zip(sizes, lengths):                               # tokens past a batch's length were cut off
            dm[a:a + n, L:] = 0
            a += n
        assert index.representations.shape == (N, 24, 32) and np.array_equal(index.mask.cpu().numpy(), dm)
        assert not dm[1].any()
        s64 = sr.maxsim_scores(pq, pd_, c["q_mask"], dm)
    else:
        assert index.representations.shape == (N, 32)
        s64 = sr.dot_scores(pq[:, 0], pd_[:, 0])
    assert np.abs(s64).max() < 2 ** 24
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    for k in (1, 10, 100, 1024):                                       # 1024 > N: padded
        val, idx = index.search(queries, k)
        torch.cuda.synchronize()
        assert val.dtype == torch.float32 and idx.dtype == torch.int32 and val.is_cuda and tuple(idx.shape) == (Q, k)
        _same((val.cpu().numpy(), idx.cpu().numpy()), sr.topk(s64.astype(np.float32), k), f"{kind} {mode} k={k}")
    ties = sum(len(np.unique(row)) < len(row) for row in s64)
    assert ties == Q, "the integer scores are meant to tie"


def _table_index(case, mode, tokens, scorer, **kw):
    from polus_amd.ir.search import CorpusIndex
    index = CorpusIndex(TableModel(case["table"], DT[mode], tokens), scorer, **kw)
    n = len(case["d_ids"])
    for b in batches(case["d_ids"], case["d_mask"], [n // 2, n - n // 2]):
        index.add(b)
    return index, {"input_ids": case["q_ids"], "attention_mask": case["q_mask"]}


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["tokens", "cls"])
def test_corpus_index_search_is_the_reference_selection_over_the_same_launches(kind, mode):
    """N(0, 1) data: scores computed here with ops.gemm / ops.maxsim_fwd over index.chunks(Q), merged by the NumPy
    reference, give exactly what search returns: selection is separated from arithmetic."""
    from polus_amd import ops
    from polus_amd.ir.training import InBatchDotScores, MaxSimScores
    tokens = kind == "tokens"
    c = token_case(**TOKEN_CASE) if tokens else cls_case(**CLS_CASE)
    Q = len(c["q_ids"])
    index, queries = _table_index(c, mode, tokens, MaxSimScores(normalize=False) if tokens else InBatchDotScores(),
                                  scratch_bytes=4 * Q * 1100)
    spans = index.chunks(Q)
    assert len(spans) >= 3
    q = index.encode_queries(queries)
    for k in KS:
        val, idx = index.search(queries, k)
        state = None
        for a, b in spans:
            s = torch.empty((Q, b - a), dtype=torch.float32, device="cuda")
            if tokens:
                am = torch.empty((Q, b - a, q.values.shape[1]), dtype=torch.int32, device="cuda")
                ops.maxsim_fwd(q.values, index.representations[a:b], q.mask, index.mask[a:b], s, am)
            else:
                ops.gemm(q, index.representations[a:b], s)
            state = sr.topk_merge(s.cpu().numpy(), np.arange(a, b), k, state)
        _same((val.cpu().numpy(), idx.cpu().numpy()), state, f"{kind} {mode} k={k}")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["tokens", "cls"])
def test_corpus_index_search_against_float64(kind, mode):
    """No case excused: every returned score within t of the float64 score of its id, every document more than 2t
    above the float64 k-th best returned, none returned more than 2t below it (t: tests/search_cases.py;
    tests/test_search_cpu.py checks these seeds on the CPU)."""
    from polus_amd.ir.training import InBatchDotScores, MaxSimScores
    tokens = kind == "tokens"
    c = token_case(**TOKEN_CASE) if tokens else cls_case(**CLS_CASE)
    index, queries = _table_index(c, mode, tokens, MaxSimScores(normalize=False) if tokens else InBatchDotScores())
    tab = rounded(c["table"], DT[mode])
    if tokens:
        s64 = sr.maxsim_scores(tab[c["q_ids"]], tab[c["d_ids"]], c["q_mask"], c["d_mask"])
        t = maxsim_tol(mode) * np.abs(s64).max()
    else:
        s64 = sr.dot_scores(tab[c["q_ids"][:, 0]], tab[c["d_ids"][:, 0]])
        t = dot_tol(CLS_CASE["E"]) * np.abs(s64).max()
    for k in KS:
        val, idx = index.search(queries, k)
        val, idx = val.cpu().numpy(), idx.cpu().numpy()
        worst = max(np.abs(val[r].astype(np.float64) - s64[r, idx[r]]).max() for r in range(len(idx)))
        print(f"{kind} {mode} k={k}: worst |score - float64| = {worst:.3e}, t = {t:.3e}")
        assert sr.check_against_float64(val, idx, s64, k, t) == []


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_normalised_maxsim_index_and_planted_corpus(mode):
    """MaxSimScores(normalize=True): the stored representations are l2norm_fwd of the projected ones, and on a corpus
    where document 10 q + 3 holds lightly perturbed copies of query q's tokens among random documents, Recall@1 is 1."""
    from polus_amd import ops
    from polus_amd.ir.metrics import RecallAtK
    from polus_amd.ir.training import MaxSimScores
    r = np.random.Generator(np.random.PCG64(31))
    Q, N, Lq, Ld, E, V = 8, 400, 8, 16, 64, 1024
    c = token_case(9, Q, N, Lq, Ld, E, V)
    qtok = r.standard_normal((Q * Lq, E)).astype(np.float32) * r.uniform(0.5, 4.0, size=(Q * Lq, 1)).astype(np.float32)
    planted = qtok + 0.05 * r.standard_normal(qtok.shape).astype(np.float32)
    c["table"] = np.concatenate([c["table"], qtok, planted], 0)
    c["q_ids"] = (V + np.arange(Q * Lq, dtype=np.int32)).reshape(Q, Lq)
    c["q_mask"][:] = 1
    pos = 10 * np.arange(Q) + 3
    c["d_ids"][pos, :Lq] = (V + Q * Lq + np.arange(Q * Lq, dtype=np.int32)).reshape(Q, Lq)
    c["d_mask"][pos, :Lq] = 1
    index, queries = _table_index(c, mode, True, MaxSimScores(normalize=True))
    x = torch.as_tensor(c["table"][c["d_ids"]]).to(DT[mode]).cuda()
    y, rn = torch.empty_like(x), torch.empty(x.shape[:2], dtype=torch.float32, device="cuda")
    ops.l2norm_fwd(x, y, rn)
    assert torch.equal(index.representations, y)
    y_ref, _ = maxsim_ref.l2norm_fwd(rounded(c["table"], DT[mode])[c["d_ids"]])
    assert_close(host(index.representations), y_ref, TOL[mode]["norm"], "stored representations")
    val, idx = index.search(queries, 5)
    m = RecallAtK(1)
    m.samples_from_batch((idx, [[int(p)] for p in pos]))
    assert m.evaluate() == 1.0
    assert (val[:, 0] <= Lq * (1 + 2e-2)).all() and (val[:, 0] > 0.9 * Lq).all()        # cosines: at most 1 per query token


@pytest.mark.parametrize("kind,mode", [("tokens", "bf16"), ("cls", "f32")])
def test_retrieval_validation_callback_end_to_end(kind, mode):
    """A tiny BERT, one epoch of EfficientDenseRetrievalTrainer.train with RetrievalValidationCallback and the three
    metrics: shared_dict["validation"][name] holds one value per metric, equal to the reference metrics of a direct
    CorpusIndex.search with the trained weights, and SaveModelCallback(strategy="best") fires."""
    from polus_amd.callbacks import SaveModelCallback
    from polus_amd.ir.metrics import MRRAtK, NDCGAtK, RecallAtK
    from polus_amd.ir.models import DualEncoder, LateInteractionDualEncoder
    from polus_amd.ir.search import CorpusIndex, RetrievalValidationCallback
    from polus_amd.ir.training import ContrastiveLoss, EfficientDenseRetrievalTrainer, InBatchDotScores, MaxSimScores
    from polus_amd.models import BertConfig, BertModel
    from polus_amd.optimizers import Adam
    from tests.test_model_gpu import load_case
    _, ocfg, params, _, _ = load_case("bert_small_b3_s48")
    cfg = BertConfig(ocfg.vocab_size, ocfg.hidden_size, ocfg.num_hidden_layers, ocfg.num_attention_heads,
                     ocfg.intermediate_size, ocfg.max_position_embeddings, ocfg.type_vocab_size)
    enc = BertModel(cfg, compute_dtype=mode); enc.load_numpy_params(params)
    r = np.random.Generator(np.random.PCG64(41))

    def batch(n, S):
        lens = r.integers(2, S + 1, size=n)
        return {"input_ids": r.integers(1, ocfg.vocab_size, size=(n, S)).astype(np.int32),
                "attention_mask": (np.arange(S) < lens[:, None]).astype(np.int32)}
    B, Sq, Sd, E, K = 6, 12, 40, 64, 5
    if kind == "tokens":
        model, scorer = LateInteractionDualEncoder(enc, projection_dim=E, compute_dtype=mode), MaxSimScores()
    else:
        model, scorer = DualEncoder(enc, projection_dim=E, compute_dtype=mode), InBatchDotScores()
    saved = []
    model.save = lambda **kw: saved.append(kw)                         # a dual encoder is not a SavableModel
    train = [(batch(B, Sq), batch(B, Sd)) for _ in range(3)]
    corpus = [batch(7, Sd), batch(5, Sd - 16)]                         # 12 documents, two adds of unequal size and length
    relevant = [set(range(8)), {0, 11}, {3: 2.0, 9: 1.0}, [5, 6, 7, 8, 9, 10, 11, 0]]
    val = [(batch(2, Sq), relevant[:2]), (batch(2, Sq), relevant[2:])]
    metrics = [RecallAtK(K), MRRAtK(K), NDCGAtK(K)]
    trainer = EfficientDenseRetrievalTrainer(model, scorer, optimizer=Adam(1e-3), loss=ContrastiveLoss(), metrics=metrics)
    before = [v.numpy().copy() for v in model.trainable_weights]
    trainer.train(train, epochs=1, callbacks=[RetrievalValidationCallback(corpus, val, K, name="val"),
                                              SaveModelCallback("best", validation_name="val", metric_name=f"Recall@{K}")])
    torch.cuda.synchronize()
    assert any(not np.array_equal(b, v.numpy()) for b, v in zip(before, model.trainable_weights)), "nothing was trained"
    res = trainer.callbacks.shared_dict["validation"]["val"]
    assert sorted(res) == sorted(m.name for m in metrics) and all(len(v) == 1 for v in res.values())
    index = CorpusIndex(model, scorer)
    for b in corpus:
        index.add(b)
    ranked = np.concatenate([index.search(q, K)[1].cpu().numpy() for q, _ in val], 0)
    assert ((ranked >= 0) & (ranked < 12)).all()
    want = {f"Recall@{K}": sr.recall_at_k(ranked, relevant, K), f"MRR@{K}": sr.mrr_at_k(ranked, relevant, K),
            f"nDCG@{K}": sr.ndcg_at_k(ranked, relevant, K)}
    for name, v in want.items():
        assert abs(res[name][0] - v) < 1e-12, (name, res[name], v)
    assert res[f"Recall@{K}"][0] > 0 and len(saved) == 1 and saved[0]["extension"] == f"_val_Recall@{K}_best"


def test_corpus_index_refusals():
    from polus_amd.ir.search import CorpusIndex
    from polus_amd.ir.training import MaxSimScores
    c = token_case(2, 4, 20, 4, 8, 32, 64)
    model = TableModel(c["table"], torch.float32, True)
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    docs = {"input_ids": c["d_ids"], "attention_mask": c["d_mask"]}
    index = CorpusIndex(model, MaxSimScores())
    with pytest.raises(ValueError, match="empty"):
        index.search(queries, 3)
    with pytest.raises(ValueError, match="post_process_logits"):
        CorpusIndex(model, MaxSimScores(), post_process_logits=lambda x: x).add(docs)
    index.add({"input_ids": c["d_ids"][:, :6], "attention_mask": c["d_mask"][:, :6]})
    with pytest.raises(ValueError, match="document length 6"):
        index.add(docs)
    assert len(index) == 20
    index.scratch_bytes = 4 * 4 - 1
    with pytest.raises(ValueError, match="scratch_bytes"):
        index.search(queries, 3)
    index.clear()
    assert len(index) == 0 and index.representations is None
    index.add(docs)                                                    # a cleared index takes a new document length
    assert index.representations.shape == (20, 8, 32)
