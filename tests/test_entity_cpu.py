"""CPU: the BIO decoding rule on hand-worked rows, parse_scheme, the host entity_counts / decode_bio of
polus_amd/ner/bio.py against the sequential decoder of tests/entity_ref.py on every case of tests/entity_cases.py, EntityF1
on host arrays, the polus.ner re-exports, and the host-side refusals of the two C entry points."""
import ctypes
import logging
import math

import numpy as np
import pytest

from tests import entity_cases as ec, entity_ref as er

TAGS = ["PAD", "O", "B-Chemical", "I-Chemical", "B-Gene", "I-Gene"]     # ids 0..5: PAD O B-c I-c B-g I-g
PAD, O, Bc, Ic, Bg, Ig = range(6)
SCHEME = [-1, -1, 0, 1, 2, 3]

# name: (a, b, mask, entities of a, entities of b, counts [T][3] = (common, n_a, n_b), stats [6])
HAND = {
    "B I I O B against itself": (
        [Bc, Ic, Ic, O, Bc], [Bc, Ic, Ic, O, Bc], None,
        [(0, 3, 0), (4, 5, 0)], [(0, 3, 0), (4, 5, 0)], [[2, 2, 2], [0, 0, 0]], [5, 0, 0, 0, 0, 0]),
    "boundary error": (
        [O, Bc, Ic, Ic, O, Bg], [O, Bc, Ic, O, O, Bg], None,
        [(1, 4, 0), (5, 6, 1)], [(1, 3, 0), (5, 6, 1)], [[0, 1, 1], [1, 1, 1]], [6, 0, 0, 0, 0, 0]),
    "type error": (
        [Bc, Ic, O, Bg], [Bg, Ig, O, Bg], None,
        [(0, 2, 0), (3, 4, 1)], [(0, 2, 1), (3, 4, 1)], [[0, 1, 0], [1, 1, 2]], [4, 0, 0, 0, 0, 0]),
    "O I I: lenient start": (
        [O, Ic, Ic], [O, Bc, Ic], None,
        [(1, 3, 0)], [(1, 3, 0)], [[1, 1, 1], [0, 0, 0]], [3, 0, 1, 0, 0, 0]),
    "B-x I-y: split in two": (
        [Bc, Ig, Ig, O], [Bc, Ic, Ic, O], None,
        [(0, 1, 0), (1, 3, 1)], [(0, 3, 0)], [[0, 1, 1], [0, 1, 0]], [4, 0, 0, 1, 0, 0]),
    "mask hole inside an entity": (           # the hole's values are never read; positions stay column indices
        [Bc, -100, Ic, O, Ig], [Bc, 99, Ic, Ic, Ig], [1, 0, 1, 1, 1],
        [(0, 3, 0), (4, 5, 1)], [(0, 4, 0), (4, 5, 1)], [[0, 1, 1], [1, 1, 1]], [4, 0, 1, 0, 0, 1]),
    "entity at the last token": (
        [O, O, Bg], [O, Bc, Ic], None,
        [(2, 3, 1)], [(1, 3, 0)], [[0, 0, 1], [0, 1, 0]], [3, 0, 0, 0, 0, 0]),
    "all-masked row": (
        [Bc, Ic, O], [Bc, Ic, O], [0, 0, 0],
        [], [], [[0, 0, 0], [0, 0, 0]], [0, 0, 0, 0, 0, 0]),
    "a hole makes neighbours": (              # B-c | hole over O | I-c goes on; B-c right after an entity starts a new one
        [Bc, O, Ic, Bc], [Bc, O, Ic, Ic], [1, 0, 1, 1],
        [(0, 3, 0), (3, 4, 0)], [(0, 4, 0)], [[0, 2, 1], [0, 0, 0]], [3, 0, 0, 0, 0, 0]),
    "rejected ids are outside": (
        [Bc, 6, Ic], [Bc, -1, Ic], None,
        [(0, 1, 0), (2, 3, 0)], [(0, 1, 0), (2, 3, 0)], [[2, 2, 2], [0, 0, 0]], [3, 2, 1, 0, 1, 0]),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_worked_rows(name):
    from polus_amd.ner import bio
    a, b, mask, ents_a, ents_b, counts, stats = HAND[name]
    a, b = np.asarray([a], np.int32), np.asarray([b], np.int32)
    m = None if mask is None else np.asarray([mask], np.int32)
    for impl_counts, impl_decode in ((lambda: er.entity_counts(a, b, SCHEME, 2, m), lambda t: er.decode(t, SCHEME, m)[0]),
                                     (lambda: bio.entity_counts(a, b, SCHEME, mask=m, num_types=2),
                                      lambda t: bio.decode_bio(t, SCHEME, mask=m)[0])):
        got_counts, got_stats = impl_counts()
        assert np.asarray(got_counts).tolist() == counts
        assert np.asarray(got_stats).tolist() == stats
        assert impl_decode(a) == [ents_a] and impl_decode(b) == [ents_b]


def test_parse_scheme():
    from polus_amd.ner import bio
    s, types = bio.parse_scheme(["PAD", "O", "B-Chemical", "I-Chemical"])          # the reference's TAG2INT
    assert s.dtype == np.int32 and s.tolist() == [-1, -1, 0, 1] and types == ["Chemical"]
    s, types = bio.parse_scheme(TAGS)
    assert s.tolist() == SCHEME and types == ["Chemical", "Gene"]
    s, types = bio.parse_scheme(["O", "I-x", "B-y", "B-x", "[CLS]", "B", "I-", "b-x", "E-x"])
    assert s.tolist() == [-1, 1, 2, 0, -1, -1, -1, -1, -1] and types == ["x", "y"]       # I-x alone defines type x
    s, types = bio.parse_scheme(["O", "B-a-b", "I-a-b"])                               # the type is all behind "B-"
    assert s.tolist() == [-1, 0, 1] and types == ["a-b"]
    for T, C in ec.SCHEMES:
        s, types = bio.parse_scheme(ec.scheme_names(T, C))
        assert np.array_equal(s, ec.scheme_table(T, C)) and len(types) == T and len(s) == C


def test_parse_scheme_and_check_scheme_refuse():
    from polus_amd.ner import bio
    with pytest.raises(ValueError, match="twice"):
        bio.parse_scheme(["O", "B-x", "I-x", "B-x"])
    with pytest.raises(ValueError, match="empty"):
        bio.parse_scheme([])
    with pytest.raises(TypeError):
        bio.parse_scheme(["O", 3])
    assert bio.check_scheme([-1, 0, 1, 2])[1] == 2
    assert bio.check_scheme([-1, -1])[1] == 1
    for bad in ([-2, 0], [], [[0, 1]], [0.0, 1.0]):
        with pytest.raises(ValueError):
            bio.check_scheme(bad)
    with pytest.raises(ValueError, match="only 1 type"):
        bio.check_scheme([-1, 0, 2], num_types=1)
    with pytest.raises(ValueError, match="shape"):
        bio.entity_counts(np.zeros((2, 3), np.int32), np.zeros((2, 4), np.int32), SCHEME)
    with pytest.raises(ValueError, match="mask"):
        bio.decode_bio(np.zeros((2, 3), np.int32), SCHEME, mask=np.ones((2, 4), np.int32))


@pytest.mark.parametrize("kind", ec.KINDS)
@pytest.mark.parametrize("TC", ec.SCHEMES, ids=[f"T{t}C{c}" for t, c in ec.SCHEMES])
def test_host_path_equals_sequential_reference(TC, kind):
    from polus_amd.ner import bio
    T, C = TC
    scheme = ec.scheme_table(T, C)
    entities = 0
    for B in ec.BS[:2]:
        for S in ec.SS:
            a, b = ec.make_pair(kind, B, S, scheme)
            if kind == "uniform" and S > 2:           # out-of-range ids at kept and at masked-out positions
                a, b = a.copy(), b.copy()
                a[0, S // 2], b[B - 1, 1] = C, -100
            for which in ec.MASKS:
                m = ec.make_mask(which, B, S)
                want_counts, want_stats = er.entity_counts(a, b, scheme, T, m)
                counts, stats = bio.entity_counts(a, b, scheme, mask=m, num_types=T)
                assert counts.tolist() == want_counts and stats.tolist() == want_stats, (B, S, which)
                want_rows, want_st = er.decode(a, scheme, m)
                rows, st = bio.decode_bio(a, scheme, mask=m)
                assert rows == want_rows and st == want_st, (B, S, which)
                entities += sum(c[0] for c in want_counts)
                M = 2
                assert bio.decode_bio(a, scheme, mask=m, max_spans=M)[0] == [r[:M] for r in want_rows]
    assert entities > 0 or kind != "edited"           # the edited copies do share entities with their gold rows


def test_planted_entities_on_the_host():
    from polus_amd.ner import bio
    scheme = ec.scheme_table(1, 4)
    for S in ec.SS:
        tags, want = ec.planted(S, scheme)
        assert er.decode(tags, scheme)[0] == want
        assert bio.decode_bio(tags, scheme)[0] == want
        n = sum(len(w) for w in want)
        assert bio.entity_counts(tags, tags, scheme)[0].tolist() == [[n, n, n]]


def test_one_dimensional_input_and_torch_host_tensors():
    import torch
    from polus_amd.ner import bio
    row = np.asarray([Bc, Ic, O, Ig], np.int64)
    assert bio.decode_bio(row, SCHEME)[0] == [[(0, 2, 0), (3, 4, 1)]]
    assert bio.decode_bio(torch.as_tensor(row), SCHEME, mask=torch.tensor([1, 1, 0, 1]))[0] == [[(0, 2, 0), (3, 4, 1)]]
    counts, _ = bio.entity_counts(torch.as_tensor(row), row, SCHEME)
    assert counts.tolist() == [[1, 1, 1], [1, 1, 1]]


def _f1(counts):
    return er.micro_f1(counts)


def test_entity_f1_accumulates_evaluates_and_resets(caplog):
    from polus_amd.ner.metrics import EntityF1
    m = EntityF1(tags=TAGS)
    assert m.name == "EntityF1" and m.last_results is None
    scheme = np.asarray(SCHEME, np.int32)
    total = [[0, 0, 0], [0, 0, 0]]
    stats = [0] * 6
    for seed, masked in ((0, False), (1, True), (2, True)):
        a, b = ec.make_pair("edited", 5, 65, scheme, seed)
        mask = ec.make_mask("holes", 5, 65, seed) if masked else None
        m.samples_from_batch((a, b, mask) if masked else (a, b))
        c, s = er.entity_counts(a, b, scheme, 2, mask)
        total = [[x + y for x, y in zip(r, q)] for r, q in zip(total, c)]
        stats = [x + y for x, y in zip(stats, s)]
    tp = total[0][0] + total[1][0]
    fn, fp = total[0][1] + total[1][1] - tp, total[0][2] + total[1][2] - tp
    assert tp > 0 and fp > 0 and fn > 0
    with caplog.at_level(logging.INFO, logger="polus_amd"):
        value = m.evaluate()
    assert isinstance(value, float) and abs(value - _f1(total)) < 1e-12
    assert abs(value - tp / (tp + 0.5 * (fp + fn))) < 1e-12
    res = m.last_results
    assert (res["tp"], res["fp"], res["fn"]) == (tp, fp, fn) and res["f1"] == value
    assert abs(res["precision"] - tp / (tp + fp)) < 1e-12 and abs(res["recall"] - tp / (tp + fn)) < 1e-12
    assert res["tags"] == stats[0]
    assert res["inside_tag_after_other_tag"] == (stats[2], stats[4])
    assert res["inside_tag_with_different_entity_type"] == (stats[3], stats[5])
    assert set(res["per_type"]) == {"Chemical", "Gene"}
    for t, name in enumerate(("Chemical", "Gene")):
        p = res["per_type"][name]
        assert (p["tp"], p["fn"], p["fp"]) == (total[t][0], total[t][1] - total[t][0], total[t][2] - total[t][0])
        assert abs(p["f1"] - _f1([total[t]])) < 1e-12
    assert any("Statistics about the BIO decoding process" in r.getMessage() and f"tags={stats[0]}" in r.getMessage()
               for r in caplog.records)
    # evaluate() has reset the counts; last_results stays
    assert m.evaluate() == 0.0 and m.last_results["tp"] == 0 and m.last_results["tags"] == 0


def test_entity_f1_zero_denominators_give_zero():
    from polus_amd.ner.metrics import EntityF1
    m = EntityF1(tags=TAGS)
    m.samples_from_batch((np.full((2, 7), O, np.int32), np.full((2, 7), O, np.int32)))
    value = m.evaluate()
    assert value == 0.0 and not math.isnan(value)
    res = m.last_results
    assert (res["precision"], res["recall"], res["f1"], res["tags"]) == (0.0, 0.0, 0.0, 14)
    assert all(p["f1"] == 0.0 for p in res["per_type"].values())
    # one side empty: precision's denominator is zero, recall's is not
    m.samples_from_batch((np.asarray([[Bc, Ic]]), np.asarray([[O, O]])))
    assert m.evaluate() == 0.0 and m.last_results["precision"] == 0.0 and m.last_results["fn"] == 1
    # a perfect batch, through reduce_f and a single row
    m2 = EntityF1(tags=TAGS, reduce_f=lambda s: (s["y"], s["p"]))
    m2.samples_from_batch({"y": np.asarray([Bc, Ic, O, Bg]), "p": np.asarray([Bc, Ic, O, Bg])})
    assert m2.evaluate() == 1.0 and m2.last_results["tp"] == 2


def test_entity_f1_tuple_order_names_precision_and_recall():
    from polus_amd.ner.metrics import EntityF1
    gold, pred = np.asarray([[Bc, Ic, O, Bg, O]]), np.asarray([[Bc, Ic, O, O, O]])
    m = EntityF1(tags=TAGS)
    m.samples_from_batch((gold, pred))
    f = m.evaluate()
    assert (m.last_results["precision"], m.last_results["recall"]) == (1.0, 0.5)
    m.samples_from_batch((pred, gold))
    assert m.evaluate() == f and (m.last_results["precision"], m.last_results["recall"]) == (0.5, 1.0)


def test_entity_f1_rejected_value_raises_at_once_on_the_host():
    from polus_amd.ner.metrics import EntityF1
    m = EntityF1(tags=TAGS)
    with pytest.raises(ValueError, match=r"1 tag value\(s\) outside \[0, 6\)"):
        m.samples_from_batch((np.asarray([[Bc, -100, O]]), np.asarray([[Bc, Ic, O]])))
    # the same value at a masked-out position is never interpreted
    m.samples_from_batch((np.asarray([[Bc, -100, O]]), np.asarray([[Bc, Ic, O]]), np.asarray([[1, 0, 1]])))
    assert m.evaluate() == 1.0


def test_entity_f1_refuses_the_reference_signature():
    from polus_amd.ner.metrics import EntityF1
    with pytest.raises(TypeError, match="corpus object model"):
        EntityF1(["corpus"])
    with pytest.raises(TypeError, match="tags"):
        EntityF1()
    with pytest.raises(ValueError, match="twice"):
        EntityF1(tags=["O", "B-x", "B-x"])


def test_polus_namespace_reexports():
    from polus.ner.bio import decode_bio, entity_counts, parse_scheme
    from polus.ner.metrics import Accuracy, EntityF1, MacroF1Score
    from polus_amd import metrics as base
    from polus_amd.ner import bio, metrics
    assert EntityF1 is metrics.EntityF1 and decode_bio is bio.decode_bio
    assert entity_counts is bio.entity_counts and parse_scheme is bio.parse_scheme
    assert MacroF1Score is base.MacroF1Score and Accuracy is base.Accuracy
    acc = Accuracy(num_classes=3)
    acc.samples_from_batch((np.asarray([[0, 1], [2, 2]]), np.asarray([[0, 1], [2, 1]])))       # [B, S] is flattened
    assert acc.evaluate() == 0.75


@pytest.fixture(scope="module")
def lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


def test_c_entry_points_refuse_on_the_host(lib):
    p = ctypes.c_void_p(256)                           # never dereferenced: every call is refused before a launch

    def counts(a=p, lda=8, b=p, ldb=8, mask=None, ldm=0, scheme=p, C=4, T=1, B=2, S=8, out=p, stats=p):
        rc = lib.polus_bio_entity_counts(a, lda, b, ldb, mask, ldm, scheme, C, T, B, S, out, stats, None)
        return rc, lib.polus_last_error()

    def spans(t=p, ldt=8, mask=None, ldm=0, scheme=p, C=4, B=2, S=8, out=p, M=8, count=p, rej=None):
        rc = lib.polus_bio_spans(t, ldt, mask, ldm, scheme, C, B, S, out, M, count, rej, None)
        return rc, lib.polus_last_error()

    for kw, word in ((dict(C=257), b"C <= 256"), (dict(C=0), b"0 < C"), (dict(T=0), b"0 < T"), (dict(T=129), b"T <= 128"),
                     (dict(S=0), b"S >= 1"), (dict(lda=7), b"strides"), (dict(ldb=7), b"strides"),
                     (dict(mask=p, ldm=7), b"ldm"), (dict(a=None), b"null"), (dict(b=None), b"null"),
                     (dict(scheme=None), b"null"), (dict(out=None), b"null"), (dict(stats=None), b"null")):
        rc, msg = counts(**kw)
        assert rc != 0 and b"polus_bio_entity_counts" in msg and word in msg, (kw, msg)
    for kw, word in ((dict(C=257), b"C <= 256"), (dict(S=0), b"S >= 1"), (dict(M=0), b"M >= 1"), (dict(ldt=7), b"ldt"),
                     (dict(mask=p, ldm=7), b"ldm"), (dict(t=None), b"null"), (dict(scheme=None), b"null"),
                     (dict(out=None), b"null"), (dict(count=None), b"null")):
        rc, msg = spans(**kw)
        assert rc != 0 and b"polus_bio_spans" in msg and word in msg, (kw, msg)
    # B == 0 is no error and launches nothing
    assert counts(B=0)[0] == 0 and spans(B=0)[0] == 0
