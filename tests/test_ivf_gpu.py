"""The inverted-list kernels on the device against the NumPy reference of tests/ivf_ref.py: polus_ivf_count / _offsets /
_fill (exact counts, offsets and lists as sets), polus_ivf_mark and polus_ivf_compact (exact sets, skipped probes,
masks, strides and padding) and polus_centroid_scores_ids (the bits of polus_centroid_scores).  Integers and bit
patterns only: no tolerance anywhere."""
import numpy as np
import pytest
import torch

from tests import ivf_ref as ir
from tests.centroid_cases import GLOBAL_SHAPES, SCORE_SHAPES, score_case
from tests.ivf_cases import LIST_SHAPES, MARK_K, MARK_N, hot_codes, ids_case, list_codes, mark_case

pytestmark = pytest.mark.gpu
POISON = 0x5A5A5A5A


def _codes_dev(codes):
    return torch.as_tensor(np.ascontiguousarray(codes).view(np.int16)).cuda()


def _i32(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.int32)).cuda()


def _build(codes, K):
    """count -> offsets -> fill on the device; every output buffer starts poisoned."""
    from polus_amd import ops
    cd = _codes_dev(codes)
    counts = torch.full((K,), 77, dtype=torch.int32, device="cuda")
    offsets = torch.full((K + 1,), 77, dtype=torch.int32, device="cuda")
    ops.ivf_count(cd, K, counts)
    ops.ivf_offsets(counts, offsets)
    P = int(offsets[K:].cpu()[0])
    cursor = torch.full((K,), 77, dtype=torch.int32, device="cuda")
    docs = torch.full((P + 4,), -3, dtype=torch.int32, device="cuda")
    ops.ivf_fill(cd, offsets, cursor, docs[:P])
    torch.cuda.synchronize()
    assert (docs[P:] == -3).all(), "entries past P were written"
    return counts.cpu().numpy(), offsets.cpu().numpy(), docs[:P].cpu().numpy()


def _check_lists(codes, K):
    want_counts, want_offsets, want_lists = ir.lists(codes, K)
    counts, offsets, docs = _build(codes, K)
    assert np.array_equal(counts, want_counts) and np.array_equal(offsets, want_offsets)
    assert len(docs) == want_offsets[K]
    for c in range(K):
        got = docs[offsets[c]:offsets[c + 1]].tolist()
        assert len(set(got)) == len(got), f"centroid {c}: an id repeats"
        assert sorted(got) == want_lists[c], f"centroid {c}"
    return counts


@pytest.mark.parametrize("N,Ld,K", LIST_SHAPES)
def test_lists_are_the_reference_as_sets(N, Ld, K):
    codes = list_codes(N, Ld, K)
    counts = _check_lists(codes, K)
    if N > 2:
        assert counts[K - 1] >= 1                                      # document 2: only its last slot present
    if Ld > K:
        assert counts.sum() < (codes < K).sum()                        # duplicates inside documents were dropped


def test_lists_with_every_document_on_one_counter():
    codes = hot_codes()
    counts = _check_lists(codes, 50)
    assert counts[0] == len(codes)


def _mark(codes, probes, qmask, N, K, lists=None, pad=2):
    """One polus_ivf_mark launch over the lists of `codes` (or the CSR pair given): the bitmap is rows 1 .. of a
    poisoned [B + 1, W + pad] buffer, so its row stride exceeds the row and every word around it can be checked."""
    from polus_amd import ops
    B, Lq, nprobe = probes.shape
    if lists is None:
        _, offsets, docs = _build(codes, K)
    else:
        offsets, docs = lists
    W = (N + 31) // 32
    buf = torch.full((B + 1, W + pad), POISON, dtype=torch.int32, device="cuda")
    wide = torch.full((B * Lq, nprobe + 3), 5, dtype=torch.int32, device="cuda")      # ldp > nprobe; 5 is a valid centroid
    wide[:, :nprobe] = _i32(probes.reshape(B * Lq, nprobe))
    ops.ivf_mark(wide[:, :nprobe], None if qmask is None else _i32(qmask), _i32(offsets), _i32(docs), N, buf[1:, :W], B, Lq)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[0] == POISON).all() and (got[1:, W:] == POISON).all(), "words outside the rows were written"
    return buf, got[1:, :W]


@pytest.mark.parametrize("N", MARK_N)
def test_mark_and_compact_are_the_reference(N):
    from polus_amd import ops
    K = MARK_K
    codes, probes, qmask = mark_case(N)
    B = probes.shape[0]
    W = (N + 31) // 32
    per_centroid = ir.lists(codes, K)[2]
    assert per_centroid[K - 2] == []
    for m in (qmask, None):
        want = ir.candidates(probes, m, per_centroid, N)
        buf, bits = _mark(codes, probes, m, N, K)
        assert np.array_equal(bits, ir.bitmap(want, N)), (N, m is None)
        if N & 31:
            assert (bits[:, W - 1] >> np.uint32(N & 31) == 0).all(), "bits >= N were set"
        most = max(1, max(len(s) for s in want))
        count = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        ops.ivf_compact(buf[1:, :W], N, count)                         # the count-only call
        assert count.cpu().tolist() == [len(s) for s in want]
        for cap in sorted({1, max(1, most // 2), most, most + 3}):
            wide = torch.full((B, cap + 2), POISON, dtype=torch.int32, device="cuda")
            count.fill_(-7)
            ops.ivf_compact(buf[1:, :W], N, count, wide[:, :cap])
            want_count, want_cand = ir.compact(bits, N, cap)
            assert np.array_equal(count.cpu().numpy(), want_count), cap
            got = wide.cpu().numpy()
            assert np.array_equal(got[:, :cap], want_cand), cap
            assert (got[:, cap:] == POISON).all(), "columns past cap were written"
            for b in range(B):
                assert want_cand[b, :min(cap, len(want[b]))].tolist() == sorted(want[b])[:cap]
        if m is not None and B > 1:
            assert len(want[1]) == 0 and (bits[1] == 0).all()          # the query without a valid token


def test_mark_skips_list_entries_outside_the_corpus():
    """Lists that do not belong to the corpus (ids -1, N and N + 3 among the entries): those entries are skipped and
    nothing outside the rows is written."""
    N, K = 70, MARK_K
    codes, probes, qmask = mark_case(N)
    _, offsets, docs = _build(codes, K)
    r = np.random.Generator(np.random.PCG64(5))
    docs = docs.copy()
    docs[r.choice(len(docs), size=len(docs) // 4, replace=False)] = r.choice([-1, N, N + 3], size=len(docs) // 4)
    per_centroid = [docs[offsets[c]:offsets[c + 1]].tolist() for c in range(K)]
    want = ir.candidates(probes, qmask, per_centroid, N)
    _, bits = _mark(codes, probes, qmask, N, K, lists=(offsets, docs))
    assert np.array_equal(bits, ir.bitmap(want, N))


@pytest.mark.parametrize("shape", SCORE_SHAPES + GLOBAL_SHAPES)
def test_scores_of_ids_have_the_bits_of_the_scan(shape):
    """N(0, 1) tables, where an order of summation would show: every (query, candidate) entry equals, as a bit pattern,
    the entry polus_centroid_scores gives that pair; ids outside [0, N) give -inf."""
    from polus_amd import ops
    B, N, Lq, Ld, K = shape
    table, qmask, codes = score_case(*shape, integer=False)
    if B > 1:
        qmask[1] = qmask[0]                                            # no empty query: every row carries bits
    cand = ids_case(B, N)
    C = cand.shape[1]
    t, qm, cd = torch.as_tensor(table).cuda(), _i32(qmask), _codes_dev(codes)
    full = torch.empty((B, N), dtype=torch.float32, device="cuda")
    ops.centroid_scores(t, qm, cd, full, B, Lq)
    wide_c = torch.full((B, C + 2), 0, dtype=torch.int32, device="cuda")               # ldc > C
    wide_c[:, :C] = _i32(cand)
    buf = torch.full((B, C + 5), -7.25, dtype=torch.float32, device="cuda")            # lds > C
    ops.centroid_scores_ids(t, qm, cd, wide_c[:, :C], buf[:, :C], B, Lq)
    torch.cuda.synchronize()
    assert (buf[:, C:] == -7.25).all(), "columns past C were written"
    got, ref = buf[:, :C].cpu().numpy(), full.cpu().numpy()
    ok = (cand >= 0) & (cand < N)
    want = np.where(ok, np.take_along_axis(ref, np.clip(cand, 0, N - 1), axis=1), -np.inf).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), shape
    assert np.isneginf(got[~ok]).all() and np.isfinite(got[ok]).all() and (Lq == 1 or np.abs(got[ok]).max() > 0)
