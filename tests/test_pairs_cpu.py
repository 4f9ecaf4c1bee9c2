"""CPU: the pair-packing rule (tests/pair_ref.py) against hand-written rows and against HF's BertTokenizer, the bucket
planner, and the host-side refusals of the three polus_pair_* entry points (no launch is made without a GPU)."""
import ctypes

import numpy as np
import pytest

from tests import pair_cases as pc
from tests import pair_ref as pr

CLS, SEP, PAD = 101, 102, 0
SP = (CLS, SEP, PAD)


def _pack(q_ids, qmask, d_ids, dmask, cand, strips, max_q, S, rows=None):
    i32 = lambda a: None if a is None else np.asarray(a, np.int32)
    return pr.pair_pack(i32(q_ids), i32(qmask), i32(d_ids), i32(dmask), i32(cand), strips, max_q, S, SP, rows)


def test_reference_rows_by_hand():
    # a hole mask on the query (tokens 11, 13, 14 kept) and a left-padded document (tokens 23, 24 kept), raw ids
    ids, tt, am, ln = _pack([[11, 12, 13, 14]], [[1, 0, 2, 1]], [[21, 22, 23, 24]], [[0, 0, 1, 1]], [[0]], (0, 0, 0, 0), 5, 10)
    assert ids.tolist() == [[CLS, 11, 13, 14, SEP, 23, 24, SEP, PAD, PAD]]
    assert tt.tolist() == [[0, 0, 0, 0, 0, 1, 1, 1, 0, 0]]
    assert am.tolist() == [[1, 1, 1, 1, 1, 1, 1, 1, 0, 0]]
    assert ln.tolist() == [8]
    # strips 1/1 take the outermost VALID tokens, not the outermost columns
    ids, tt, am, ln = _pack([[7, 11, 12, 8, 0]], [[1, 1, 1, 1, 0]], [[0, 7, 21, 8]], [[0, 1, 1, 1]], [[0]], (1, 1, 1, 1), 5, 8)
    assert ids.tolist() == [[CLS, 11, 12, SEP, 21, SEP, PAD, PAD]] and ln.tolist() == [6]
    assert tt.tolist() == [[0, 0, 0, 0, 1, 1, 0, 0]]


def test_reference_empty_query_and_oversized_strips():
    # nq = 0: an all-zero query mask; the row still starts cls sep
    ids, tt, am, ln = _pack([[11, 12]], [[0, 0]], [[21, 22, 23]], None, [[0]], (0, 0, 0, 0), 4, 8)
    assert ids.tolist() == [[CLS, SEP, 21, 22, 23, SEP, PAD, PAD]] and ln.tolist() == [6]
    assert tt.tolist() == [[0, 0, 1, 1, 1, 1, 0, 0]] and am.tolist() == [[1] * 6 + [0, 0]]
    # strips larger than the rows leave none: head + tail = 4 > 3 tokens, and 8 + 8 against 2
    ids, _, am, ln = _pack([[11, 12, 13]], None, [[21, 22]], None, [[0]], (2, 2, 8, 8), 4, 7)
    assert ids.tolist() == [[CLS, SEP, SEP, PAD, PAD, PAD, PAD]] and ln.tolist() == [3] and am.sum() == 3
    # max_q = 0 drops the query as well
    ids, _, _, ln = _pack([[11, 12, 13]], None, [[21, 22]], None, [[0]], (0, 0, 0, 0), 0, 5)
    assert ids.tolist() == [[CLS, SEP, 21, 22, SEP]] and ln.tolist() == [5]


def test_reference_both_truncations_missing_candidates_and_repeats():
    q = [[11, 12, 13, 14, 15]]
    d = [[21, 22, 23, 24, 25, 26], [31, 32, 33, 34, 35, 36]]
    # max_q = 3 cuts the query to its first 3, S = 8 leaves the document 8 - 3 - 3 = 2: the row is full, no padding
    ids, tt, am, ln = _pack(q, None, d, None, [[1]], (0, 0, 0, 0), 3, 8)
    assert ids.tolist() == [[CLS, 11, 12, 13, SEP, 31, 32, SEP]] and ln.tolist() == [8]
    assert tt.tolist() == [[0, 0, 0, 0, 0, 1, 1, 1]] and am.tolist() == [[1] * 8]
    # missing candidates (-1 and N) give cls q sep sep; rows picks pairs in any order, one of them twice
    ids, tt, am, ln = _pack(q, None, d, None, [[0, -1, 2]], (0, 0, 0, 0), 2, 7, rows=[2, 0, 1, 0])
    empty = [CLS, 11, 12, SEP, SEP, PAD, PAD]
    full = [CLS, 11, 12, SEP, 21, 22, SEP]
    assert ids.tolist() == [empty, full, empty, full] and ln.tolist() == [5, 7, 5, 7]
    assert tt[0].tolist() == [0, 0, 0, 0, 1, 0, 0] and am[0].tolist() == [1, 1, 1, 1, 1, 0, 0]
    assert pr.pair_lengths(None, (1, 5), None, (2, 6), np.array([[0, -1, 2]]), (0, 0, 0, 0), 2, 7, rows=[2, 0, 1, 0]).tolist() == [5, 7, 5, 7]
    out = pr.scatter_scores([1.0, 2.0], np.array([[0, -1, 2]]), 2, np.full((1, 3), 9.0, np.float32), rows=[1, 0])
    assert out.tolist() == [[2.0, -np.inf, 9.0]]


@pytest.mark.parametrize("mask_kind", pc.MASKS)
def test_reference_invariants_over_the_gpu_cases(mask_kind):
    """Every case the GPU test runs: a row is cls + kept query + sep + kept document + sep + pad, the kept tokens are a
    prefix of the stripped valid tokens, and no row is fully masked."""
    for (Lq, Ld, S, B, n), strips, rows_kind in [(s, t, r) for s in pc.shapes()[::5] for t in pc.STRIPS for r in pc.ROWS]:
        c = pc.make_case(Lq, Ld, S, B, n, mask_kind, rows_kind)
        ids, tt, am, ln = pr.pair_pack(c["q_ids"], c["qmask"], c["d_ids"], c["dmask"], c["cand"], strips, c["max_q"], S,
                                       pc.SPECIAL, c["rows"])
        assert (ln >= 3).all() and (ln <= S).all() and (am.sum(1) == ln).all()
        assert (ids[:, 0] == pc.SPECIAL[0]).all() and ((ids == pc.SPECIAL[1]).sum(1) == 2).all()
        assert ((ids == pc.SPECIAL[2]) == (am == 0)).all() and (tt[am == 0] == 0).all()
        assert (ln == pr.pair_lengths(c["qmask"], (B, Lq), c["dmask"], (pc.N_DOCS, Ld), c["cand"], strips, c["max_q"], S,
                                      c["rows"])).all()


def test_reference_matches_hf_bert_tokenizer(tmp_path):
    transformers = pytest.importorskip("transformers")
    words = [f"w{i}" for i in range(40)]
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words
    (tmp_path / "vocab.txt").write_text("\n".join(vocab) + "\n")
    tok = transformers.BertTokenizer(str(tmp_path / "vocab.txt"), do_lower_case=True)
    special = (tok.cls_token_id, tok.sep_token_id, tok.pad_token_id)
    r = np.random.Generator(np.random.PCG64(4))
    text = lambda k: " ".join(words[int(i)] for i in r.integers(0, len(words), size=k))
    queries = [text(k) for k in (1, 3, 6)]
    # no empty document: the tokenizer takes an empty second text as "no pair" and writes one [SEP]; the rule's
    # empty-document row `cls q sep sep` (a missing candidate) is pinned by the hand-written rows above
    docs = [text(k) for k in (1, 2, 9, 14, 30)]
    max_q = 6                                             # the queries are within max_q: only_second never cuts them
    Lq, Ld = 10, 34

    def padded(texts, L):
        e = tok(texts, padding="max_length", max_length=L)
        return np.asarray(e["input_ids"], np.int32), np.asarray(e["attention_mask"], np.int32)
    q_ids, qmask = padded(queries, Lq)
    d_ids, dmask = padded(docs, Ld)
    cand = np.array([[0, 1, 2, 3, 4]] * len(queries), np.int32)
    for S in (12, 16, 40):                                # the documents of 9+ tokens are truncated at 12 and 16
        ids, tt, am, _ = pr.pair_pack(q_ids, qmask, d_ids, dmask, cand, (1, 1, 1, 1), max_q, S, special)
        for b, q in enumerate(queries):
            for j, d in enumerate(docs):
                e = tok(q, d, truncation="only_second", max_length=S, padding="max_length")
                p = b * len(docs) + j
                assert ids[p].tolist() == e["input_ids"], (S, q, d)
                assert tt[p].tolist() == e["token_type_ids"], (S, q, d)
                assert am[p].tolist() == e["attention_mask"], (S, q, d)


def test_plan_buckets():
    from polus_amd.ir.cross import plan_buckets
    r = np.random.Generator(np.random.PCG64(11))
    for lengths, budget, round_to, max_length in [
            (r.integers(3, 257, size=500), 4096, 64, 256), (r.integers(3, 50, size=37), 100, 16, 48),
            (np.array([256, 3, 3, 200]), 100, 64, 256),   # budget below one row: single-row buckets
            (np.full(9, 17), 64, 1, None), (np.array([5]), 1 << 20, 64, 256)]:
        plan = plan_buckets(lengths, budget, round_to, max_length)
        again = plan_buckets(lengths.copy(), budget, round_to, max_length)
        assert [(s, rows.tolist()) for s, rows in plan] == [(s, rows.tolist()) for s, rows in again]
        seen = np.concatenate([rows for _, rows in plan])
        assert sorted(seen.tolist()) == list(range(lengths.size)), "every pair exactly once"
        assert seen.dtype == np.int32
        # descending length, ties by pair index
        key = [(-int(lengths[p]), int(p)) for p in seen]
        assert key == sorted(key)
        for S, rows in plan:
            assert rows.size >= 1 and (lengths[rows] <= S).all()
            assert rows.size * S <= budget or rows.size == 1
            assert S % round_to == 0 or S == max_length
            assert max_length is None or S <= max_length
            assert S - int(lengths[rows[0]]) < round_to
    assert plan_buckets(np.zeros(0, np.int64), 10) == []
    for bad in (lambda: plan_buckets([3.5], 10), lambda: plan_buckets([3], 0), lambda: plan_buckets([300], 10, 64, 256),
                lambda: plan_buckets([0], 10)):
        with pytest.raises(ValueError):
            bad()


@pytest.fixture(scope="module")
def lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


P = ctypes.c_void_p(16)       # a non-null pointer that is never dereferenced: every call below is refused before a launch
GOOD = dict(q_ids=P, ldq=8, qmask=P, ldqm=8, d_ids=P, ldd=9, dmask=P, lddm=9, cand=P, ldc=4, rows=None, R=8, B=2, n=4, N=5,
            Lq=8, Ld=9, q_head=1, q_tail=1, d_head=1, d_tail=1, max_q=6, S=16, cls=101, sep=102, pad=0, input_ids=P,
            token_type_ids=P, attention_mask=P, ldo=16, length=P, stream=None)
LENGTHS_ARGS = ("qmask", "ldqm", "dmask", "lddm", "cand", "ldc", "rows", "R", "B", "n", "N", "Lq", "Ld", "q_head", "q_tail",
                "d_head", "d_tail", "max_q", "S", "length", "stream")
PACK_ARGS = ("q_ids", "ldq", "qmask", "ldqm", "d_ids", "ldd", "dmask", "lddm", "cand", "ldc", "rows", "R", "B", "n", "N", "Lq",
             "Ld", "q_head", "q_tail", "d_head", "d_tail", "max_q", "S", "cls", "sep", "pad", "input_ids", "token_type_ids",
             "attention_mask", "ldo", "length", "stream")
# (changed arguments, a word of the message, applies to polus_pair_lengths too)
BAD = [(dict(cand=None), "null", True), (dict(q_ids=None), "null", False), (dict(d_ids=None), "null", False),
       (dict(input_ids=None), "null", False), (dict(token_type_ids=None), "null", False),
       (dict(attention_mask=None), "null", False),
       (dict(R=0), ">= 1", True), (dict(B=0), ">= 1", True), (dict(n=0), ">= 1", True), (dict(N=0), ">= 1", True),
       (dict(Lq=0), ">= 1", True), (dict(Ld=0), ">= 1", True),
       (dict(B=65536, n=32768, ldc=32768), "2^31", True),
       (dict(ldc=3), "ldc", True), (dict(ldqm=7), "stride", True), (dict(lddm=8), "stride", True),
       (dict(ldq=7), "stride", False), (dict(ldd=8), "stride", False), (dict(ldo=15), "ldo", False),
       (dict(q_head=9), "strip", True), (dict(q_tail=-1), "strip", True), (dict(d_head=-1), "strip", True),
       (dict(d_tail=9), "strip", True), (dict(max_q=-1), "max_q", True), (dict(S=8), "max_q + 3", True),
       (dict(max_q=2147483647, S=2147483647), "max_q + 3", True)]


def test_pair_entry_points_refuse_bad_arguments_on_the_host(lib):
    for change, word, both in BAD:
        a = dict(GOOD, **change)
        rc = lib.polus_pair_pack(*[a[k] for k in PACK_ARGS])
        assert rc != 0 and word.encode() in lib.polus_last_error(), ("pack", change, lib.polus_last_error())
        assert b"polus_pair_pack" in lib.polus_last_error()
        if both:
            rc = lib.polus_pair_lengths(*[a[k] for k in LENGTHS_ARGS])
            assert rc != 0 and word.encode() in lib.polus_last_error(), ("lengths", change, lib.polus_last_error())
            assert b"polus_pair_lengths" in lib.polus_last_error()
    rc = lib.polus_pair_lengths(*[dict(GOOD, length=None)[k] for k in LENGTHS_ARGS])
    assert rc != 0 and b"null" in lib.polus_last_error()
    # NULL masks, rows and polus_pair_pack's length are legal: with them the first complaint is about something else
    a = dict(GOOD, qmask=None, dmask=None, ldqm=0, lddm=0, rows=None, length=None, S=8)
    assert lib.polus_pair_pack(*[a[k] for k in PACK_ARGS]) != 0 and b"max_q + 3" in lib.polus_last_error()
    good = dict(s=P, rows=None, cand=P, ldc=4, R=8, B=2, n=4, N=5, out=P, ldo=4, stream=None)
    order = ("s", "rows", "cand", "ldc", "R", "B", "n", "N", "out", "ldo", "stream")
    for change, word in [(dict(s=None), "null"), (dict(cand=None), "null"), (dict(out=None), "null"), (dict(R=0), ">= 1"),
                         (dict(B=0), ">= 1"), (dict(n=0), ">= 1"), (dict(N=0), ">= 1"), (dict(ldc=3), "stride"),
                         (dict(ldo=3), "stride"), (dict(B=65536, n=32768, ldc=32768, ldo=32768), "2^31")]:
        a = dict(good, **change)
        rc = lib.polus_pair_scatter_scores(*[a[k] for k in order])
        assert rc != 0 and word.encode() in lib.polus_last_error(), ("scatter", change, lib.polus_last_error())


def test_ops_check_host_rows():
    from polus_amd import ops
    assert ops._pair_rows(None, 2, 4) == (None, 8)
    for rows, distinct in (([8], False), ([-1], False), ([0, 1, 0], True), ([], False), ([0.5], False)):
        with pytest.raises(ValueError):
            ops._pair_rows(np.asarray(rows), 2, 4, distinct=distinct)
