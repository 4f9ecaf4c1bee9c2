"""On the device: polus_bio_entity_counts and polus_bio_spans against the sequential decoder of tests/entity_ref.py on
host copies (exact integer equality), EntityF1's device path against its host path, the NER head end to end, and the
C ABI's refusals.  Shapes, row kinds and masks: tests/entity_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import entity_cases as ec, entity_ref as er
from tests.util import dev

pytestmark = pytest.mark.gpu
GUARD, FILL = 16, 0x5A5A5A5A
PAD_COLS = 5                                       # unused columns behind a row: row stride S + 5
JUNK = (1000, -100, 256, -1, 2 ** 31 - 1)          # ids outside [0, C) for every scheme
SHAPES = [(B, S) for B in ec.BS for S in ec.SS]
_CASES = {}


def _combos():
    """(kind, mask, (T, C)) for every kind x mask, the schemes taken in turn so that each meets every kind and mask."""
    return [(kind, which, ec.SCHEMES[(ki + mi) % len(ec.SCHEMES)])
            for ki, kind in enumerate(ec.KINDS) for mi, which in enumerate(ec.MASKS)]


def _case(B, S, kind, which, TC):
    """Host arrays of a case (masked-out positions overwritten with out-of-range ids: they must never be read) and the
    reference's answers, computed once and shared by the tests below (nothing writes to them)."""
    key = (B, S, kind, which, TC)
    if key not in _CASES:
        T, C = TC
        scheme = ec.scheme_table(T, C)
        a, b = ec.make_pair(kind, B, S, scheme)
        m = ec.make_mask(which, B, S)
        if m is not None:
            a, b = a.copy(), b.copy()
            a[m == 0], b[m == 0] = JUNK[1], JUNK[0]
        rows_a, st_a = er.decode(a, scheme, m)
        rows_b, st_b = er.decode(b, scheme, m)
        counts, stats = er.counts_from_decoded(rows_a, st_a, rows_b, st_b, T)
        _CASES[key] = dict(T=T, C=C, scheme=scheme, a=a, b=b, m=m, rows_a=rows_a, counts=counts, stats=stats)
    return _CASES[key]


def _wide(x, junk):
    """x [B, S] as the leading columns of a device buffer [B, S + PAD_COLS] whose other columns hold `junk`."""
    buf = torch.full((x.shape[0], x.shape[1] + PAD_COLS), junk, dtype=torch.int32, device="cuda")
    buf[:, :x.shape[1]] = torch.as_tensor(np.ascontiguousarray(x))
    return buf[:, :x.shape[1]]


def _guarded(n):
    """A device int32 buffer of n zeros with GUARD fill values behind them: (the n elements, the whole buffer)."""
    buf = torch.full((n + GUARD,), FILL, dtype=torch.int32, device="cuda")
    buf[:n] = 0
    return buf[:n], buf


def _guard_ok(buf, n):
    return bool((buf[n:] == FILL).all())


def _counts(a, b, scheme, T, m=None, wide=True):
    """One ops.bio_entity_counts call into zeroed, guarded accumulators: (counts [T][3], stats [6]) as lists."""
    from polus_amd import ops
    put = (lambda x, j: _wide(x, j)) if wide else (lambda x, j: dev(x))
    counts, cbuf = _guarded(T * 3)
    stats, sbuf = _guarded(6)
    ops.bio_entity_counts(put(a, JUNK[0]), put(b, JUNK[1]), dev(scheme), counts.view(T, 3), stats,
                          mask=None if m is None else put(m, 1))
    torch.cuda.synchronize()
    assert _guard_ok(cbuf, T * 3) and _guard_ok(sbuf, 6)
    return counts.view(T, 3).cpu().tolist(), stats.cpu().tolist()


def _spans(tags, scheme, m=None, M=None):
    """One ops.bio_spans call: (spans [B, M, 3] with FILL in untouched slots, count [B], rejected) on the host."""
    from polus_amd import ops
    B, S = tags.shape
    M = S if M is None else M
    sbuf = torch.full((B * M * 3 + GUARD,), FILL, dtype=torch.int32, device="cuda")
    cbuf = torch.full((B + GUARD,), FILL, dtype=torch.int32, device="cuda")
    rej, rbuf = _guarded(1)
    ops.bio_spans(_wide(tags, JUNK[2]), dev(scheme), sbuf[:B * M * 3].view(B, M, 3), cbuf[:B],
                  mask=None if m is None else _wide(m, 1), rejected=rej)
    torch.cuda.synchronize()
    assert _guard_ok(sbuf, B * M * 3) and _guard_ok(cbuf, B) and _guard_ok(rbuf, 1)
    return sbuf[:B * M * 3].view(B, M, 3).cpu().numpy(), cbuf[:B].cpu().numpy(), int(rej.item())


def _check_spans(spans, count, rows, M):
    for r, want in enumerate(rows):
        assert count[r] == len(want), r                        # the true number, also above M
        k = min(len(want), M)
        assert [tuple(e) for e in spans[r, :k].tolist()] == want[:k], r     # in order of start
        assert (spans[r, k:] == FILL).all(), r                  # slots behind them are not touched


# ---------------------------------------------------------------- polus_bio_entity_counts
@pytest.mark.parametrize("B,S", SHAPES)
def test_entity_counts_equal_reference(B, S):
    """Every kind of row under every mask, the schemes in turn (T = 1 / C = 4, T = 3, T = 128 / C = 256); row strides
    larger than S with out-of-range ids in the unused columns and at masked-out positions: rejected stays 0."""
    common = 0
    for kind, which, TC in _combos():
        c = _case(B, S, kind, which, TC)
        counts, stats = _counts(c["a"], c["b"], c["scheme"], c["T"], c["m"])
        assert counts == c["counts"] and stats == c["stats"], (kind, which, TC)
        assert stats[1] == 0
        common += sum(row[0] for row in counts)
    assert common > 0 or S < 3


@pytest.mark.parametrize("S", ec.SS)
def test_entity_counts_planted_entities(S):
    """One entity per row that starts at 63, ends at 63, ends at 64, spans the row, sits at the last token: against
    itself all common; against a copy whose every entity is one token shorter or longer, none."""
    scheme = ec.scheme_table(1, 4)
    tags, want = ec.planted(S, scheme)
    n = sum(len(w) for w in want)
    counts, stats = _counts(tags, tags, scheme, 1)
    assert counts == [[n, n, n]] and stats == [5 * S, 0, 0, 0, 0, 0]
    other = tags.copy()
    o, inside = int(np.nonzero(scheme == -1)[0][0]), int(np.nonzero(scheme == 1)[0][0])
    for r, ents in enumerate(want):
        for s, e, _ in ents:
            if e < S:
                other[r, e] = inside                           # one token longer
            elif e - s > 1:
                other[r, e - 1] = o                            # one token shorter
            else:
                other[r, s] = o                                # a single token at the row's end: gone
    counts, _ = _counts(tags, other, scheme, 1)
    assert counts == er.entity_counts(tags, other, scheme, 1)[0] and counts[0][0] == 0 and counts[0][1] == n


def test_entity_counts_accumulate():
    from polus_amd import ops
    c1, c2 = _case(5, 129, "edited", "holes", (3, 8)), _case(5, 129, "uniform", "none", (3, 8))
    counts, cbuf = _guarded(9)
    stats, sbuf = _guarded(6)
    scheme = dev(c1["scheme"])
    for c in (c1, c2):
        ops.bio_entity_counts(dev(c["a"]), dev(c["b"]), scheme, counts.view(3, 3), stats,
                              mask=None if c["m"] is None else dev(c["m"]))
    torch.cuda.synchronize()
    assert counts.view(3, 3).cpu().tolist() == (np.asarray(c1["counts"]) + np.asarray(c2["counts"])).tolist()
    assert stats.cpu().tolist() == (np.asarray(c1["stats"]) + np.asarray(c2["stats"])).tolist()
    assert _guard_ok(cbuf, 9) and _guard_ok(sbuf, 6)


@pytest.mark.parametrize("S", (1, 65, 300))
def test_entity_counts_reject_out_of_range_ids_at_kept_positions(S):
    """Counted per tensor, and decoded as outside (so the entity around one is cut in two)."""
    T, C = 3, 8
    scheme = ec.scheme_table(T, C)
    a, b = ec.make_pair("edited", 5, S, scheme)
    a, b = a.copy(), b.copy()
    m = ec.make_mask("holes", 5, S)
    m[0] = 1
    a[0, S // 2], a[4, 0], b[0, S // 2], b[2, S - 1] = C, -1, 2 ** 31 - 1, -100
    want_counts, want_stats = er.entity_counts(a, b, scheme, T, m)
    counts, stats = _counts(a, b, scheme, T, m)
    assert counts == want_counts and stats == want_stats and stats[1] >= 2


def test_entity_counts_single_row_and_contiguous_inputs():
    c = _case(1, 300, "edited", "prefix", (1, 4))
    assert _counts(c["a"], c["b"], c["scheme"], 1, c["m"], wide=False) == (c["counts"], c["stats"])


# ---------------------------------------------------------------- polus_bio_spans
@pytest.mark.parametrize("B,S", SHAPES)
def test_spans_equal_reference(B, S):
    for kind, which, TC in _combos():
        c = _case(B, S, kind, which, TC)
        spans, count, rejected = _spans(c["a"], c["scheme"], c["m"])
        _check_spans(spans, count, c["rows_a"], S)
        assert rejected == 0


@pytest.mark.parametrize("M", (1, 3))
def test_spans_with_fewer_slots_than_entities(M):
    c = _case(5, 129, "uniform", "holes", (3, 8))
    assert max(len(r) for r in c["rows_a"]) > 3
    spans, count, _ = _spans(c["a"], c["scheme"], c["m"], M=M)
    _check_spans(spans, count, c["rows_a"], M)


@pytest.mark.parametrize("S", ec.SS)
def test_spans_planted_entities_and_rejected(S):
    scheme = ec.scheme_table(1, 4)
    tags, want = ec.planted(S, scheme)
    spans, count, rejected = _spans(tags, scheme)
    _check_spans(spans, count, want, S)
    assert rejected == 0
    tags[3, S // 2] = 4                                        # out of range inside the entity that spans the row
    spans, count, rejected = _spans(tags, scheme)
    _check_spans(spans, count, er.decode(tags, scheme)[0], S)
    assert rejected == 1


def test_decode_bio_on_device_tensors():
    from polus_amd.ner import bio
    c = _case(5, 65, "edited", "holes", (3, 8))
    spans, count = bio.decode_bio(dev(c["a"]).long(), c["scheme"], mask=c["m"])      # int64 tags, host mask
    assert spans.is_cuda and count.is_cuda and tuple(spans.shape) == (5, 65, 3)
    host_rows, _ = bio.decode_bio(c["a"], c["scheme"], mask=c["m"])
    assert host_rows == c["rows_a"]
    spans, count = spans.cpu().numpy(), count.cpu().numpy()
    for r, want in enumerate(c["rows_a"]):
        assert count[r] == len(want) and [tuple(e) for e in spans[r, :len(want)].tolist()] == want
        assert (spans[r, len(want):] == -1).all()


# ---------------------------------------------------------------- EntityF1
def _batches():
    T, C = 3, 8
    return [_case(5, 129, "edited", "holes", (T, C)), _case(67, 65, "wellformed", "prefix", (T, C)),
            _case(5, 300, "edited", "none", (T, C)), _case(67, 64, "uniform", "zero_row", (T, C))]


def test_entity_f1_device_path_equals_host_path_and_mixes():
    from polus_amd.ner.metrics import EntityF1
    names = ec.scheme_names(3, 8)
    on_dev, on_host, mixed = EntityF1(tags=names), EntityF1(tags=names), EntityF1(tags=names)
    total = np.zeros((3, 3), np.int64)
    for k, c in enumerate(_batches()):
        host = (c["a"], c["b"]) if c["m"] is None else (c["a"], c["b"], c["m"])
        device = tuple(dev(x) for x in host)
        on_host.samples_from_batch(host)
        on_dev.samples_from_batch(device)
        mixed.samples_from_batch(device if k % 2 else host)
        total += np.asarray(c["counts"])
    # the accumulators stay on the device until evaluate(): nothing has reached the host side of the metric
    assert on_dev._dev_counts.is_cuda and on_dev._dev_stats.is_cuda
    assert on_dev._host_counts.sum() == 0 and on_dev._host_stats.sum() == 0
    want = er.micro_f1(total.tolist())
    assert 0.0 < want < 1.0
    values = [m.evaluate() for m in (on_dev, on_host, mixed)]
    assert all(abs(v - want) < 1e-12 for v in values)
    assert on_dev.last_results == on_host.last_results == mixed.last_results
    assert on_dev.last_results["tp"] == int(total[:, 0].sum())
    assert on_dev._dev_counts is None and on_dev.evaluate() == 0.0                 # reset


def test_entity_f1_device_path_raises_on_rejected_values_in_evaluate():
    from polus_amd.ner.metrics import EntityF1
    m = EntityF1(tags=ec.scheme_names(1, 4))
    a = torch.tensor([[2, 3, 1, -100]], dtype=torch.int32, device="cuda")
    m.samples_from_batch((a, a))                                                   # counted on the device: no error yet
    with pytest.raises(ValueError, match=r"2 tag value\(s\) outside \[0, 4\)"):
        m.evaluate()
    m.reset()
    m.samples_from_batch((a, a, torch.tensor([[1, 1, 1, 0]], device="cuda")))       # masked out: never interpreted
    assert m.evaluate() == 1.0 and m.last_results["tags"] == 3


def test_entity_f1_end_to_end_with_the_ner_head():
    """baselineNER_MLP_CRF.inference (device int32 [B, S]) with device labels and a mask into EntityF1; one row alone
    through the [S] form."""
    from polus_amd.ner.metrics import EntityF1
    from polus_amd.ner.models import baselineNER_MLP_CRF
    B, S, C = 6, 48, 4
    names = ["PAD", "O", "B-Chemical", "I-Chemical"]
    scheme = np.asarray([-1, -1, 0, 1], np.int32)
    r = np.random.Generator(np.random.PCG64(77))
    model = baselineNER_MLP_CRF(sequence_length=S, output_classes=C, input_dim=32)
    x = r.standard_normal((B, S, 32)).astype(np.float32)
    pred = model.inference(x)
    assert pred.is_cuda and pred.dtype == torch.int32 and tuple(pred.shape) == (B, S)
    labels = ec.wellformed_rows(B, S, scheme)
    mask = ec.make_mask("prefix", B, S)
    metric = EntityF1(tags=names)
    metric.samples_from_batch((dev(labels), pred, dev(mask)))
    metric.samples_from_batch((dev(labels[1]), pred[1]))
    c1 = er.entity_counts(labels, pred.cpu().numpy(), scheme, 1, mask)[0]
    c2 = er.entity_counts(labels[1:2], pred[1:2].cpu().numpy(), scheme, 1)[0]
    total = [[x + y for x, y in zip(c1[0], c2[0])]]
    assert total[0][1] > 0
    assert abs(metric.evaluate() - er.micro_f1(total)) < 1e-12
    assert (metric.last_results["tp"], metric.last_results["fn"]) == (total[0][0], total[0][1] - total[0][0])


# ---------------------------------------------------------------- refusals
def test_c_abi_refuses_before_any_launch():
    from polus_amd import _lib
    lib = _lib.load()
    scheme = dev(ec.scheme_table(1, 4))
    a = dev(ec.uniform_rows(2, 8, ec.scheme_table(1, 4)))
    counts, cbuf = _guarded(3)
    stats, sbuf = _guarded(6)
    spans = torch.full((2 * 8 * 3,), FILL, dtype=torch.int32, device="cuda")
    count = torch.full((2,), FILL, dtype=torch.int32, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream

    def entity_counts(tags=a, lda=8, C=4, T=1):
        rc = lib.polus_bio_entity_counts(None if tags is None else P(tags), lda, P(a), 8, None, 0, P(scheme), C, T, 2, 8,
                                         P(counts), P(stats), st)
        return rc, lib.polus_last_error()

    def bio_spans(tags=a, ldt=8, C=4, M=8):
        rc = lib.polus_bio_spans(None if tags is None else P(tags), ldt, None, 0, P(scheme), C, 2, 8, P(spans), M, P(count),
                                 None, st)
        return rc, lib.polus_last_error()

    for kw in (dict(C=257), dict(T=0), dict(lda=7), dict(tags=None)):
        rc, msg = entity_counts(**kw)
        assert rc != 0 and b"polus_bio_entity_counts" in msg, kw
    for kw in (dict(C=257), dict(M=0), dict(ldt=7), dict(tags=None)):
        rc, msg = bio_spans(**kw)
        assert rc != 0 and b"polus_bio_spans" in msg, kw
    torch.cuda.synchronize()
    # nothing ran: the accumulators are still zero and the outputs still hold their fill value
    assert counts.sum().item() == 0 and stats.sum().item() == 0 and _guard_ok(cbuf, 3) and _guard_ok(sbuf, 6)
    assert bool((spans == FILL).all()) and bool((count == FILL).all())
    assert entity_counts()[0] == 0 and bio_spans()[0] == 0                          # the same calls, unbroken, do run
    torch.cuda.synchronize()
    assert stats[0].item() == 16 and bool((count != FILL).all())
