"""GPU: polus_pair_lengths / polus_pair_pack / polus_pair_scatter_scores bit for bit against tests/pair_ref.py over the
cross product of tests/pair_cases.py.  Every tensor is a view of a wider buffer pre-filled with a sentinel: the
surplus columns, the rows behind the last one and the tails must come back untouched."""
import numpy as np
import pytest
import torch

from tests import pair_cases as pc
from tests import pair_ref as pr

pytestmark = pytest.mark.gpu
SENTINEL = -77


def _wide(a, extra_cols, fill):
    """(buffer, view): the 2-d host array `a` in the top-left corner of a device buffer with `extra_cols` more columns
    and one more row, the rest `fill`."""
    t = torch.as_tensor(np.ascontiguousarray(a))
    buf = torch.full((a.shape[0] + 1, a.shape[1] + extra_cols), fill, dtype=t.dtype).cuda()
    view = buf[:a.shape[0], :a.shape[1]]
    view.copy_(t)
    return buf, view


def _out(R, S, extra_cols=4):
    buf = torch.full((R + 1, S + extra_cols), SENTINEL, dtype=torch.int32, device="cuda")
    return buf, buf[:R, :S]


def _untouched(buf, R, S):
    h = buf.cpu().numpy()
    return (h[R:] == SENTINEL).all() and (h[:R, S:] == SENTINEL).all()


@pytest.mark.parametrize("strips", pc.STRIPS, ids=lambda s: f"strip{s[0]}")
@pytest.mark.parametrize("mask_kind", pc.MASKS)
def test_pair_kernels_match_the_reference(mask_kind, strips):
    from polus_amd import ops
    seen_missing = seen_trunc_both = 0
    for (Lq, Ld, S, B, n) in pc.shapes():
        for rows_kind in pc.ROWS:
            c = pc.make_case(Lq, Ld, S, B, n, mask_kind, rows_kind)
            what = (Lq, Ld, S, B, n, mask_kind, strips, rows_kind)
            max_q = c["max_q"]
            ref = pr.pair_pack(c["q_ids"], c["qmask"], c["d_ids"], c["dmask"], c["cand"], strips, max_q, S, pc.SPECIAL, c["rows"])
            R = ref[0].shape[0]
            _, q_ids = _wide(c["q_ids"], 3, 7)
            _, d_ids = _wide(c["d_ids"], 2, 7)
            qmask = None if c["qmask"] is None else _wide(c["qmask"], 5, 1)[1]
            dmask = None if c["dmask"] is None else _wide(c["dmask"], 1, 1)[1]
            _, cand = _wide(c["cand"], 1, 0)
            rows = None if c["rows"] is None else torch.as_tensor(c["rows"]).cuda()
            (bi, oi), (bt, ot), (bm, om) = _out(R, S), _out(R, S), _out(R, S)
            ln_pack = torch.full((R + 2,), SENTINEL, dtype=torch.int32, device="cuda")
            ln_only = torch.full((R + 2,), SENTINEL, dtype=torch.int32, device="cuda")
            ops.pair_pack(q_ids, qmask, d_ids, dmask, cand, oi, ot, om, strips, max_q, pc.SPECIAL, rows=rows, length=ln_pack)
            ops.pair_lengths((B, Lq), qmask, (pc.N_DOCS, Ld), dmask, cand, ln_only, strips, max_q, S, rows=rows)
            for name, got, want in (("input_ids", oi, ref[0]), ("token_type_ids", ot, ref[1]), ("attention_mask", om, ref[2])):
                assert np.array_equal(got.cpu().numpy(), want), (name, what)
            for buf in (bi, bt, bm):
                assert _untouched(buf, R, S), ("wrote outside the S columns", what)
            for name, ln in (("pack", ln_pack), ("lengths", ln_only)):
                h = ln.cpu().numpy()
                assert np.array_equal(h[:R], ref[3]) and (h[R:] == SENTINEL).all(), (name, what)
            # a second call without `length` leaves the same rows
            (bi2, oi2), (bt2, ot2), (bm2, om2) = _out(R, S, 0), _out(R, S, 0), _out(R, S, 0)
            ops.pair_pack(q_ids, qmask, d_ids, dmask, cand, oi2, ot2, om2, strips, max_q, pc.SPECIAL, rows=rows)
            assert torch.equal(oi2, oi) and torch.equal(ot2, ot) and torch.equal(om2, om), what
            # scatter: distinct rows only
            srows = None if c["rows"] is None else np.unique(c["rows"])[::-1].copy()
            nr = B * n if srows is None else srows.size
            s = np.arange(1, nr + 1, dtype=np.float32) * 0.5
            out0 = np.full((B, n), 9.25, np.float32)
            bo, out = _wide(out0, 2, 9.25)
            ops.pair_scatter_scores(torch.as_tensor(s).cuda(), cand, pc.N_DOCS, out, rows=None if srows is None else torch.as_tensor(srows).cuda())
            want = pr.scatter_scores(s, c["cand"], pc.N_DOCS, out0, srows)
            assert np.array_equal(out.cpu().numpy(), want), ("scatter", what)
            hb = bo.cpu().numpy()
            assert (hb[B:] == 9.25).all() and (hb[:B, n:] == 9.25).all(), ("scatter wrote outside", what)
            seen_missing += int(((c["cand"] < 0) | (c["cand"] >= pc.N_DOCS)).any())
            seen_trunc_both += int((ref[3] == S).any() and Lq > max_q)
    assert seen_missing > 20 and seen_trunc_both > 5, (seen_missing, seen_trunc_both)


def test_host_rows_are_checked_and_device_rows_taken_as_they_are():
    from polus_amd import ops
    c = pc.make_case(5, 7, 16, 3, 4, "prefix", "all")
    q_ids, d_ids, cand = (torch.as_tensor(c[k]).cuda() for k in ("q_ids", "d_ids", "cand"))
    out = [torch.empty((2, 16), dtype=torch.int32, device="cuda") for _ in range(3)]
    with pytest.raises(ValueError):
        ops.pair_pack(q_ids, None, d_ids, None, cand, *out, (0, 0, 0, 0), 6, pc.SPECIAL, rows=np.array([0, 12]))
    ops.pair_pack(q_ids, None, d_ids, None, cand, *out, (0, 0, 0, 0), 6, pc.SPECIAL, rows=np.array([11, 0]))
    ref = pr.pair_pack(c["q_ids"], None, c["d_ids"], None, c["cand"], (0, 0, 0, 0), 6, 16, pc.SPECIAL, [11, 0])
    assert np.array_equal(out[0].cpu().numpy(), ref[0])
    s = torch.ones(2, device="cuda")
    with pytest.raises(ValueError):
        ops.pair_scatter_scores(s, cand, pc.N_DOCS, torch.zeros((3, 4), device="cuda"), rows=np.array([1, 1]))
