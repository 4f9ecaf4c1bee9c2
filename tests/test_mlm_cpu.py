"""CPU: the masked-LM pieces that need no GPU -- the tolerance meta-test of the wide loss (the bounds of
tests/mlm_cases.py hold an f32 restatement of the kernel with room to spare and see the faults that matter), the host-only
route query, `mask_tokens`, and the checkpoint mapping of the HF masked-LM head."""
import numpy as np
import pytest
import torch

from tests import mlm_cases as mc
from tests import mlm_ref as mr
from tests.util import elem_err


@pytest.fixture(scope="module")
def ops():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------- tolerance meta-test
@pytest.mark.parametrize("V", [7, 257, 2049, 30522, 131075])
def test_wide_loss_bounds_hold_f32_arithmetic_and_see_faults(V):
    labels = mc.labels_for(V)
    for scale in (1.0, 4.0, 12.0):
        x = mc.logits_for(V, scale).astype(np.float32).astype(np.float64)
        ref_loss, ref_d, counted, rejected = mr.xent_wide(x, labels)
        assert (counted, rejected) == (3, 1)
        loss, d = mr.xent_wide_f32(x, labels)
        e = elem_err(d, ref_d, mc.DL_RTOL["f32"], mc.DL_FLOOR)
        e_loss = abs(loss - ref_loss) / abs(ref_loss)
        _, d_col = mr.xent_wide_f32(x, labels, drop_last_column=True)
        _, d_cnt = mr.xent_wide_f32(x, labels, wrong_count=True)
        e_col = elem_err(d_col, ref_d, mc.DL_RTOL["f32"], mc.DL_FLOOR)
        e_cnt = elem_err(d_cnt, ref_d, mc.DL_RTOL["f32"], mc.DL_FLOOR)
        print(f"[mlm] V={V} scale={scale:g}: f32 restatement {e:.4f} x bound, loss rel err {e_loss:.2e}; "
              f"dropped last column {e_col:.1f} x, wrong count {e_cnt:.1f} x")
        assert e < 0.05, (V, scale, e)
        assert e_loss < 2e-5, (V, scale, e_loss)                       # TOL[float32] of tests/util.py
        assert e_col >= 7.0 and e_cnt >= 7.0, (V, scale, e_col, e_cnt)


def test_case_rows_are_what_the_docstring_says():
    for dt in ("f32", "bf16"):
        E = 16 // mc.ESIZE[dt]
        for V in mc.WIDTHS[dt]:
            for scale in mc.SCALES:
                x = torch.as_tensor(np.array(mc.logits_for(V, scale, dt))).to(torch.bfloat16 if dt == "bf16" else torch.float32).double().numpy()
                if V > 1:
                    assert x[2].argmax() == V - 1 and x[2, V - 1] - np.sort(x[2])[-2] >= 0.5
                if V >= E:
                    assert x[3].argmax() % E == E - 1
                assert (np.abs(x[5]) > 9e3).all()
    assert {int(i) for i in mc.GATHER_IDX} >= {-1, 0, mc.GATHER_T - 1} and len(set(mc.GATHER_IDX.tolist())) < len(mc.GATHER_IDX)


# ------------------------------------------------------------------------------------------------- route query (host only)
def test_route_query_runs_without_a_gpu(ops):
    def route(dtype, V, ld, rows=5):
        buf = torch.empty((rows, ld), dtype=dtype)
        assert buf.data_ptr() % 16 == 0
        return ops.softmax_xent_wide_route(buf[:, :V])
    for dtype, es in ((torch.float32, 4), (torch.bfloat16, 2)):
        r = route(dtype, 30522, 30528)
        assert (r.path, r.vec16, r.lds_bytes) == ("staged", True, (30522 * es + 15) // 16 * 16)
        cut = mc.STAGE_BYTES // es
        assert route(dtype, cut, cut).path == "staged" and route(dtype, cut, cut).lds_bytes == mc.STAGE_BYTES
        r = route(dtype, cut + 1, cut + 16 // es)
        assert (r.path, r.vec16, r.lds_bytes) == ("streaming", True, 0)
    assert not route(torch.bfloat16, 30522, 30522).vec16           # odd rows start on a 4-byte boundary
    assert not route(torch.float32, 30522, 30522).vec16
    assert route(torch.float32, 30524, 30524).vec16
    # a misaligned base switches the wide accesses off as well
    buf = torch.empty(4 + 8 * 64, dtype=torch.float32)
    assert not ops.softmax_xent_wide_route(buf[1:1 + 8 * 64].view(8, 64)).vec16
    assert ops.softmax_xent_wide_route(buf[4:4 + 8 * 64].view(8, 64)).vec16


def test_wide_loss_argument_validation_happens_on_the_host(ops):
    import ctypes
    from polus_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)
    assert lib.polus_softmax_xent_wide(0, p, 8, p, p, p, 8, None, 4, 9, p, 1 << 20, None) != 0
    assert b"bad shape" in lib.polus_last_error()
    assert lib.polus_softmax_xent_wide(0, p, 16, p, p, p, 8, None, 4, 8, p, 1 << 20, None) != 0
    assert b"in place" in lib.polus_last_error()
    assert lib.polus_softmax_xent_wide(0, p, 8, p, p, ctypes.c_void_p(4096), 8, None, 4, 8, p, 8, None) != 0
    assert b"workspace" in lib.polus_last_error()
    assert lib.polus_softmax_xent_wide(2, p, 8, p, p, p, 8, None, 4, 8, p, 1 << 20, None) != 0
    assert b"dtype" in lib.polus_last_error()
    assert lib.polus_gather_rows(0, p, 4, p, ctypes.c_void_p(4096), 8, 3, 5, 8, None) != 0
    assert b"bad shape" in lib.polus_last_error()
    assert lib.polus_gather_rows(0, p, 8, p, p, 8, 3, 5, 8, None) != 0
    assert b"y == x" in lib.polus_last_error()
    assert lib.polus_inverse_map(p, 0, ctypes.c_void_p(4096), 5, None) != 0
    assert b"bad shape" in lib.polus_last_error()
    assert lib.polus_softmax_xent_wide_workspace_bytes(2560) == 16 + 2560 * 4
    from polus_amd._lib import PolusHipError
    t = torch.zeros(4, 8)
    with pytest.raises(PolusHipError):
        ops.softmax_xent_wide(t, torch.zeros(4, dtype=torch.int32), torch.zeros(1))
    with pytest.raises(PolusHipError):
        ops.gather_rows(t, torch.zeros(2, dtype=torch.int32), torch.zeros(2, 8))


# ------------------------------------------------------------------------------------------------- the reference itself
def test_reference_matches_hf_bert_for_masked_lm():
    """tests/mlm_ref.py (oracle.bert encoder + head + wide loss + tied gradient) against HF BertForMaskedLM in float64:
    loss and every gradient to 1e-9 relative, the tied word-table gradient included, on a batch in which one sequence has
    no masked position and one has a padded tail."""
    transformers = pytest.importorskip("transformers")
    from oracle import bert as ob
    from polus_amd.checkpoint import hf_state_to_params
    V, H, L, A, I, S = 97, 64, 1, 1, 128, 16
    hcfg = transformers.BertConfig(vocab_size=V, hidden_size=H, num_hidden_layers=L, num_attention_heads=A, intermediate_size=I,
                                   max_position_embeddings=S, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                                   hidden_act="gelu", attn_implementation="eager")
    torch.manual_seed(0)
    hf = transformers.BertForMaskedLM(hcfg).double().train()
    with torch.no_grad():                                      # biases and LayerNorm parameters start at 0 / 1: give them signal
        for n, q in hf.named_parameters():
            if n.endswith("bias") or "LayerNorm" in n:
                q.add_(0.05 * torch.randn_like(q))
    ocfg = ob.BertConfig(V, H, L, A, I, S)
    p = hf_state_to_params({k: v.detach().numpy() for k, v in hf.state_dict().items()}, L)
    assert {"mlm.dense.w", "mlm.dense.b", "mlm.ln.g", "mlm.ln.b", "mlm.bias"} <= set(p)
    ids, mask, tt, pos, lab = mr.mlm_batch(ocfg, 3, S, 4)
    assert (pos[1] < 0).all() and mask[2, -1] == 0
    hf_labels = np.full((3, S), -100, np.int64)
    for b in range(3):
        for j, l in zip(pos[b], lab[b]):
            if j >= 0:
                hf_labels[b, j] = l
    out = hf(input_ids=torch.as_tensor(ids).long(), attention_mask=torch.as_tensor(mask).long(),
             token_type_ids=torch.as_tensor(tt).long(), labels=torch.as_tensor(hf_labels))
    out.loss.backward()
    loss, logits, g = mr.mlm_fwd_bwd(p, ocfg, ids, mask, tt, pos, lab)
    rel = lambda a, r: float(np.abs(np.asarray(a) - np.asarray(r)).max() / (np.abs(np.asarray(r)).max() + 1e-300))
    print(f"[mlm] HF loss {out.loss.item():.12f}, reference {loss:.12f}")
    assert abs(loss - out.loss.item()) <= 1e-9 * abs(out.loss.item())
    hf_logits = out.logits.detach().numpy()
    for b in range(3):
        for k, j in enumerate(pos[b]):
            if j >= 0:
                assert rel(logits[b, k], hf_logits[b, j]) <= 1e-9
    hg = hf_state_to_params({n: q.grad.numpy() for n, q in hf.named_parameters()}, L)
    assert set(hg) == {k for k in g if "/" not in k}
    for k in sorted(hg):
        e = rel(g[k], hg[k])
        print(f"[mlm] HF grad {k}: rel err {e:.2e}")
        assert e <= 1e-9, (k, e)
    assert rel(g["emb.word/embedding"], hg["emb.word"]) > 1e-3 and rel(g["emb.word/decoder"], hg["emb.word"]) > 1e-3


# ------------------------------------------------------------------------------------------------- mask_tokens
SPECIAL = (0, 1, 2, 3, 4)


def _mask(ids, att, seed=0, **kw):
    from polus_amd.data import mask_tokens
    a = dict(mask_id=4, vocab_size=30000, special_ids=SPECIAL, max_predictions=20, p=0.15, rng=np.random.Generator(np.random.PCG64(seed)))
    a.update(kw)
    return mask_tokens(ids, att, **a)


def _corpus(B=64, S=128, seed=1):
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = rng.integers(5, 30000, size=(B, S)).astype(np.int32)
    ids[:, 0], ids[:, 60] = 1, 2
    att = np.ones((B, S), np.int32)
    lens = rng.integers(8, S + 1, size=B)
    att[np.arange(S)[None] >= lens[:, None]] = 0
    ids[att == 0] = 0
    return ids, att, lens


def test_mask_tokens_positions_counts_and_determinism():
    ids, att, lens = _corpus()
    out = _mask(ids, att, seed=5)
    again = _mask(ids, att, seed=5)
    assert all(np.array_equal(a, b) for a, b in zip(out, again)) and not np.array_equal(out[1], _mask(ids, att, seed=6)[1])
    new, pos, lab = out
    assert new.dtype == pos.dtype == lab.dtype == np.int32 and pos.shape == lab.shape == (64, 20)
    assert new is not ids and np.array_equal(ids, _corpus()[0]), "the input was modified"
    for b in range(64):
        n = int(((att[b] != 0) & ~np.isin(ids[b], SPECIAL)).sum())
        k = min(20, max(1, int(round(0.15 * n))))
        used = pos[b] >= 0
        assert used.sum() == k and used[:k].all() and (pos[b, k:] == -1).all() and (lab[b, k:] == -1).all()
        chosen = pos[b, :k]
        assert (np.diff(chosen) > 0).all()                              # distinct, ascending
        assert (att[b, chosen] != 0).all() and not np.isin(ids[b, chosen], SPECIAL).any()
        assert np.array_equal(lab[b, :k], ids[b, chosen])
        rest = np.ones(128, bool)
        rest[chosen] = False
        assert np.array_equal(new[b, rest], ids[b, rest])
        assert not np.isin(new[b, chosen][new[b, chosen] != 4], SPECIAL).any()   # a random replacement is never special
    assert (_mask(ids, att, max_predictions=3)[1] >= 0).sum(1).max() == 3        # the cap
    only_special = np.full((1, 8), 1, np.int32)
    _, pos0, lab0 = _mask(only_special, np.ones((1, 8), np.int32))
    assert (pos0 == -1).all() and (lab0 == -1).all()


def test_mask_tokens_80_10_10_split():
    ids, att, _ = _corpus(B=200, S=128, seed=2)
    att[:] = 1
    n_mask = n_same = n_rand = 0
    seed = 0
    while n_mask + n_same + n_rand < 20000:
        new, pos, lab = _mask(ids, att, seed=seed, max_predictions=128)
        seed += 1
        for b in range(ids.shape[0]):
            c = pos[b][pos[b] >= 0]
            v = new[b, c]
            n_mask += int((v == 4).sum())
            n_same += int((v == ids[b, c]).sum())
            n_rand += int(((v != 4) & (v != ids[b, c])).sum())
    n = n_mask + n_same + n_rand
    for what, got, q in (("mask", n_mask, 0.8), ("unchanged", n_same, 0.1), ("random", n_rand, 0.1)):
        sigma = (n * q * (1 - q)) ** 0.5
        print(f"[mlm] {what}: {got} of {n} ({got / n:.4f}), {abs(got - n * q) / sigma:.2f} sigma")
        assert abs(got - n * q) <= 4 * sigma          # a random id equal to the original (3e-5 of the 10 %) is far inside


# ------------------------------------------------------------------------------------------------- checkpoint mapping
def test_checkpoint_mapping_of_the_masked_lm_head(tmp_path):
    from oracle import bert as ob
    from polus_amd.checkpoint import hf_state_to_params, read_local_hf_checkpoint
    ocfg = ob.BertConfig(97, 64, 1, 1, 128, 16)
    p = mr.mlm_params(ocfg)
    path = mr.write_hf_checkpoint(str(tmp_path / "tied"), ocfg, p)
    cfg, got = read_local_hf_checkpoint(path)
    assert set(got) == set(p)
    for k in p:
        assert np.array_equal(got[k], p[k].astype(np.float32)), k
    # the old gamma / beta spellings
    st = mr.hf_state(ocfg, p)
    old = {k.replace("LayerNorm.weight", "LayerNorm.gamma").replace("LayerNorm.bias", "LayerNorm.beta"): v for k, v in st.items()}
    got_old = hf_state_to_params(old, 1)
    assert np.array_equal(got_old["mlm.ln.g"], got["mlm.ln.g"]) and np.array_equal(got_old["mlm.ln.b"], got["mlm.ln.b"])
    # an untied decoder is an error
    with pytest.raises(ValueError, match="untied"):
        hf_state_to_params(mr.hf_state(ocfg, p, tied=False), 1)
    # a state without cls.* maps exactly as before: the encoder's names, nothing else
    plain = hf_state_to_params(mr.hf_state(ocfg, p, with_head=False), 1)
    assert set(plain) == {k for k in p if not k.startswith("mlm.")}
    for k in plain:
        assert np.array_equal(plain[k], got[k])
