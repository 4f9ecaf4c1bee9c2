"""MaxSim (token-level late interaction) and row L2 normalisation kernels (polus_amd/csrc/maxsim.hip) against the
float64 reference of tests/maxsim_ref.py, both engines: parity over ragged / holed / empty masks, exact scores and
the lowest-j tie rule on small-integer data, argmax agreement away from near-ties, every output written, bitwise
reproducibility, and the host-side refusals."""
import numpy as np
import pytest
import torch

from tests import maxsim_ref as ref
from tests.maxsim_cases import BENCH, MASKS, SHAPES, TOL, gap_floor, make_case
from tests.util import assert_close, host, relerr, rounded

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _dev(a, dtype=None):
    if a is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda()


def _fwd(q, d, qm, dm, mode, lds=None):
    from polus_amd import ops
    B, Lq, _ = q.shape
    N = d.shape[0]
    qt, dt = _dev(q, DT[mode]), _dev(d, DT[mode])
    score = torch.full((B, lds or N), float("nan"), dtype=torch.float32, device="cuda")
    am = torch.full((B, N, Lq), 12345, dtype=torch.int32, device="cuda")
    ops.maxsim_fwd(qt, dt, _dev(qm), _dev(dm), score, am)
    return qt, dt, score, am


def _bwd(qt, dt, ds, am):
    from polus_amd import ops
    dq = torch.full_like(qt, float("nan"))
    dd = torch.full_like(dt, float("nan"))
    ops.maxsim_bwd(qt, dt, ds, am, dq, dd)
    return dq, dd


def _check_case(shape, masks, mode):
    q, d, qm, dm = make_case(shape, masks)
    B, k, Lq, Ld, E = shape
    N = (1 + k) * B
    qr, dr = rounded(q, DT[mode]), rounded(d, DT[mode])
    qt, dt, score, am = _fwd(q, d, qm, dm, mode)
    torch.cuda.synchronize()
    s_ref, am_ref = ref.maxsim_fwd(qr, dr, qm, dm)
    got, amg = host(score), am.cpu().numpy()
    assert np.isfinite(got).all()
    assert_close(got, s_ref, TOL[mode]["score"], f"{shape} {masks} score")
    # argmax: -1 exactly where the reference has -1; equal wherever the top-two gap is clear of rounding
    assert np.array_equal(amg < 0, am_ref < 0)
    gap = ref.top2_gap(qr, dr, qm, dm)
    clear = (am_ref >= 0) & (gap > gap_floor(qr, dr))
    assert np.array_equal(amg[clear], am_ref[clear]), f"{shape} {masks}: argmax differs at {int((amg[clear] != am_ref[clear]).sum())}"
    assert ((amg >= -1) & (amg < Ld)).all()
    if dm is not None:                                              # never a masked document token
        c_idx = np.broadcast_to(np.arange(N)[None, :, None], amg.shape)
        assert (dm[c_idx[amg >= 0], amg[amg >= 0]] != 0).all()
    # backward, checked against the reference evaluated with the device's argmax
    r = np.random.Generator(np.random.PCG64(5))
    ds = r.standard_normal((B, N)).astype(np.float32)
    dq, dd = _bwd(qt, dt, _dev(ds), am)
    torch.cuda.synchronize()
    dq_ref, dd_ref = ref.maxsim_bwd(qr, dr, ds, amg)
    dqh, ddh = host(dq), host(dd)
    assert np.isfinite(dqh).all() and np.isfinite(ddh).all()
    assert_close(dqh, dq_ref, TOL[mode]["grad"], f"{shape} {masks} dQ")
    assert_close(ddh, dd_ref, TOL[mode]["grad"], f"{shape} {masks} dD")
    if qm is not None:
        assert (dqh[qm == 0] == 0).all(), "masked query rows of dQ must be exactly 0"
    if dm is not None:
        assert (ddh[dm == 0] == 0).all(), "masked document rows of dD must be exactly 0"
    return relerr(got, s_ref), relerr(dqh, dq_ref), relerr(ddh, dd_ref)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("masks", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxsim_parity(shape, masks, mode):
    _check_case(shape, masks, mode)


@pytest.mark.parametrize("masks", ["none", "ragged"])
def test_maxsim_parity_bench_shape_bf16(masks):
    _check_case(BENCH, masks, "bf16")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_maxsim_exact_small_integers_and_lowest_j_ties(mode):
    """Integer data: every dot product and score is exact in both engines, so scores equal the reference bit for
    bit and so does the argmax, ties included (asymmetric data: a swapped fragment layout fails)."""
    r = np.random.Generator(np.random.PCG64(9))
    B, N, Lq, Ld, E = 3, 4, 20, 40, 64
    q = r.integers(-3, 4, size=(B, Lq, E)).astype(np.float32)
    d = r.integers(-3, 4, size=(N, Ld, E)).astype(np.float32)
    q[:, :, 0] += np.arange(Lq)[None] % 5                          # asymmetric in token and feature
    d[:, :, 1] -= np.arange(Ld)[None] % 3
    d[:, 25] = d[:, 7]                                              # duplicated document tokens: j = 7 must win
    d[:, 33] = d[:, 7]
    d[1, 12:20] = d[1, 3]                                           # a run of duplicates straddling a 16-row tile
    d[2] = 0.0                                                      # all-zero document: every j ties -> 0
    qm = np.ones((B, Lq), np.int32); qm[1, 15:] = 0
    dm = np.ones((N, Ld), np.int32); dm[3, :5] = 0; dm[3, 30:] = 0
    for qmask, dmask in ((None, None), (qm, dm)):
        qt, dt, score, am = _fwd(q, d, qmask, dmask, mode)
        torch.cuda.synchronize()
        s_ref, am_ref = ref.maxsim_fwd(q, d, qmask, dmask)
        assert np.array_equal(score.cpu().numpy(), s_ref.astype(np.float32)), "scores must be exact"
        assert np.array_equal(am.cpu().numpy(), am_ref)
        amg = am.cpu().numpy()
        assert (amg[:, 2] == 0).all() if qmask is None else (amg[:, 2][qm == 1] == 0).all()
        best = amg[:, 0]                                            # duplicates of token 7 never win over 7
        assert not np.isin(best, [25, 33]).any()


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_maxsim_strided_destination_and_determinism(mode):
    """Scores written into column block [B:2B] of a wider matrix leave the other columns untouched; two runs give
    bitwise-equal scores, argmax, dQ and dD."""
    from polus_amd import ops
    shape = (8, 1, 32, 180, 128)
    q, d, qm, dm = make_case(shape, "ragged")
    B, N = 8, 16
    qt, dt = _dev(q, DT[mode]), _dev(d, DT[mode])
    big = torch.full((B, 3 * N + 5), -7.25, dtype=torch.float32, device="cuda")
    am = torch.empty((B, N, 32), dtype=torch.int32, device="cuda")
    ops.maxsim_fwd(qt, dt, _dev(qm), _dev(dm), big[:, N:2 * N], am)
    _, _, score, am2 = _fwd(q, d, qm, dm, mode)
    torch.cuda.synchronize()
    bh = big.cpu().numpy()
    assert (bh[:, :N] == -7.25).all() and (bh[:, 2 * N:] == -7.25).all()
    assert torch.equal(big[:, N:2 * N], score) and torch.equal(am, am2)
    ds = torch.as_tensor(np.random.Generator(np.random.PCG64(3)).standard_normal((B, N)).astype(np.float32)).cuda()
    dq1, dd1 = _bwd(qt, dt, ds, am)
    dq2, dd2 = _bwd(qt, dt, ds, am)
    wide = torch.zeros((B, 2 * N), dtype=torch.float32, device="cuda")
    wide[:, :N] = ds
    dq3, dd3 = _bwd(qt, dt, wide[:, :N], am)                       # strided dscore
    torch.cuda.synchronize()
    for a, b in ((dq1, dq2), (dd1, dd2), (dq1, dq3), (dd1, dd3)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_l2norm_matches_reference(mode):
    from polus_amd import ops
    r = np.random.Generator(np.random.PCG64(4))
    for rows, E in ((7, 128), (300, 32), (33, 256), (5, 96)):
        x = (r.standard_normal((rows, E)) * r.uniform(0.1, 10, size=(rows, 1))).astype(np.float32)
        x[1] = 0.0                                                  # zero row: y = 0, dx = dy / eps
        x[2] = 1e-14                                                # |x| below eps
        dy = r.standard_normal((rows, E)).astype(np.float32)
        xr, dyr = rounded(x, DT[mode]), rounded(dy, DT[mode])
        xt = _dev(x, DT[mode])
        y = torch.full_like(xt, float("nan"))
        rn = torch.full((rows,), float("nan"), dtype=torch.float32, device="cuda")
        ops.l2norm_fwd(xt, y, rn)
        dx = torch.full_like(xt, float("nan"))
        ops.l2norm_bwd(y, rn, _dev(dy, DT[mode]), dx)
        torch.cuda.synchronize()
        y_ref, rn_ref = ref.l2norm_fwd(xr)
        ok = np.ones(rows, bool); ok[[1, 2]] = False
        assert_close(host(y)[ok], y_ref[ok], TOL[mode]["norm"], "y")
        assert (host(y)[1] == 0).all()
        assert_close(host(rn)[ok], rn_ref[ok], 1e-6, "rnorm")
        assert host(rn)[1] == np.float32(1e12)
        # backward from the device's y (the forward output as stored)
        dx_ref = ref.l2norm_bwd(xr, dyr)
        assert_close(host(dx)[ok], dx_ref[ok], 2 * TOL[mode]["norm"] if mode == "f32" else 1.5e-2, "dx")
        assert_close(host(dx)[[1, 2]], dyr[[1, 2]] / 1e-12, 1e-2 if mode == "bf16" else 1e-6, "dx of rows below eps")


def _refused(fn, msg):
    from polus_amd._lib import PolusHipError
    with pytest.raises(PolusHipError) as e:
        fn()
    assert msg in str(e.value), str(e.value)


def test_maxsim_refusals_name_their_limit():
    """Device tensors of the invalid shapes, sized for the call they make: a refusal that did not fire would still
    launch on valid memory."""
    from polus_amd import ops

    def call(B, N, Lq, Ld, E):
        q = torch.zeros((B, Lq, E), dtype=torch.float32, device="cuda")
        d = torch.zeros((N, Ld, E), dtype=torch.float32, device="cuda")
        s = torch.empty((B, N), dtype=torch.float32, device="cuda")
        am = torch.empty((B, N, Lq), dtype=torch.int32, device="cuda")
        return lambda: ops.maxsim_fwd(q, d, None, None, s, am), lambda: ops.maxsim_bwd(q, d, s, am, torch.empty_like(q), torch.empty_like(d))

    for shape, msg in (((1, 1, 1, 1, 48), "multiple of 32"), ((1, 1, 1, 1, 288), "multiple of 32"),
                       ((1, 1, 513, 1, 32), "Lq <= 512"), ((1, 1, 1, 513, 32), "Ld <= 512"),
                       ((65536, 1, 1, 1, 32), "B <= 65535"), ((1, 65536, 1, 1, 32), "N <= 65535")):
        f, b = call(*shape)
        _refused(f, msg)
        _refused(b, msg)
        torch.cuda.synchronize()
    # B*N*Lq >= 2^31: the argmax alone is 8.6 GB, allocated but never written
    f, b = call(2049, 2049, 512, 1, 32)
    _refused(f, "2^31")
    _refused(b, "2^31")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def test_maxsim_refuses_cpu_tensors():
    from polus_amd import ops
    from polus_amd._lib import PolusHipError
    q = torch.zeros((1, 1, 32))
    with pytest.raises(PolusHipError):
        ops.maxsim_fwd(q, q, None, None, torch.zeros(1, 1), torch.zeros(1, 1, 1, dtype=torch.int32))
    with pytest.raises(PolusHipError):
        ops.l2norm_fwd(q, q, torch.zeros(1))


@pytest.mark.parametrize("k", [0, 2])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_late_interaction_trainer_step(mode, k):
    """EfficientDenseRetrievalTrainer with LateInteractionDualEncoder + MaxSimScores + ContrastiveLoss on two frozen
    BERT encoders (ragged masks, k explicit negatives): loss and projection gradients against the NumPy BERT oracle
    -> projection -> normalise -> MaxSim -> softmax CE (backward with the device's argmax), the encoders untouched,
    and the first Adam step."""
    from oracle import bert as ob
    from oracle import losses as ol
    from polus_amd.ir.models import LateInteractionDualEncoder, TokenReps
    from polus_amd.ir.training import ContrastiveLoss, EfficientDenseRetrievalTrainer, MaxSimScores
    from polus_amd.models import BertConfig, BertModel
    from polus_amd.optimizers import Adam
    from tests.test_model_gpu import load_case
    g, ocfg, params, _, _ = load_case("bert_small_b3_s48")
    cfg = BertConfig(ocfg.vocab_size, ocfg.hidden_size, ocfg.num_hidden_layers, ocfg.num_attention_heads,
                     ocfg.intermediate_size, ocfg.max_position_embeddings, ocfg.type_vocab_size)
    qenc = BertModel(cfg, compute_dtype=mode); qenc.load_numpy_params(params)
    denc = BertModel(cfg, compute_dtype=mode); denc.load_numpy_params(params)
    B, Sq, Sd, E = 6, 12, 40, 64
    r = np.random.Generator(np.random.PCG64(21 + k))

    def batch(n, S, shape):
        ids = r.integers(1, ocfg.vocab_size, size=shape + (S,)).astype(np.int32)
        lens = r.integers(1, S + 1, size=shape)
        return {"input_ids": ids, "attention_mask": (np.arange(S) < lens[..., None]).astype(np.int32)}
    q, d = batch(B, Sq, (B,)), batch(B, Sd, (B,))
    neg = batch(B, Sd, (B, k)) if k else None
    model = LateInteractionDualEncoder(qenc, denc, projection_dim=E, compute_dtype=mode)
    scorer = MaxSimScores()
    before = (qenc.arena.params.clone(), denc.arena.params.clone())
    w = {v.name: v.numpy().astype(np.float64) for v in model.trainable_weights}
    opt = Adam(1e-3)
    trainer = EfficientDenseRetrievalTrainer(model, scorer, optimizer=opt, loss=ContrastiveLoss())
    reps = trainer.forward_without_grads(q, d, neg) if k else None
    if k:
        assert all(isinstance(x, TokenReps) for x in reps)
    loss = float(trainer.train_step(q, d, neg) if k else trainer.train_step(q, d))
    torch.cuda.synchronize()
    assert torch.equal(before[0], qenc.arena.params) and torch.equal(before[1], denc.arena.params)
    # oracle
    n = [v.name for v in model.trainable_weights]
    wq, bq, wd, bd = (w[x] for x in n)
    hq = ob.bert_fwd(params, ocfg, q["input_ids"], q["attention_mask"])[0]
    dids, dmask = [d["input_ids"]], [d["attention_mask"]]
    for i in range(k):
        dids.append(neg["input_ids"][:, i]); dmask.append(neg["attention_mask"][:, i])
    hd = np.concatenate([ob.bert_fwd(params, ocfg, a, m)[0] for a, m in zip(dids, dmask)], 0)
    dm = np.concatenate(dmask, 0)
    qm = q["attention_mask"]
    pq, pd_ = hq @ wq.T + bq, hd @ wd.T + bd
    yq, _ = ref.l2norm_fwd(pq)
    yd, _ = ref.l2norm_fwd(pd_)
    s_ref, _ = ref.maxsim_fwd(yq, yd, qm, dm)
    loss_ref, ds = ol.sparse_softmax_xent_fwd(s_ref, np.arange(B))
    assert abs(loss - loss_ref) < (1e-4 if mode == "f32" else 5e-2) * max(1.0, abs(loss_ref)), (loss, loss_ref)
    am = scorer.argmax.cpu().numpy()
    assert am.shape == (B, (1 + k) * B, Sq)
    assert (am[np.broadcast_to(qm[:, None, :] == 0, am.shape)] == -1).all()
    gq, gd = ref.maxsim_bwd(yq, yd, ds, am)
    dq, dd = ref.l2norm_bwd(pq, gq), ref.l2norm_bwd(pd_, gd)
    grads = {v.name: v.grad.detach().cpu().numpy().astype(np.float64) for v in model.trainable_weights}
    tol = 5e-4 if mode == "f32" else 8e-2
    assert_close(grads[n[0]], dq.reshape(-1, E).T @ hq.reshape(-1, hq.shape[-1]), tol, "query projection dW")
    assert_close(grads[n[1]], dq.reshape(-1, E).sum(0), tol, "query projection db")
    assert_close(grads[n[2]], dd.reshape(-1, E).T @ hd.reshape(-1, hd.shape[-1]), tol, "document projection dW")
    assert_close(grads[n[3]], dd.reshape(-1, E).sum(0), tol, "document projection db")
    # the first Adam step from the device's gradients (Keras Adam, t = 1)
    b1, b2, eps, lr = 0.9, 0.999, 1e-7, 1e-3
    lr_t = lr * np.sqrt(1 - b2) / (1 - b1)
    for v in model.trainable_weights:
        gr = grads[v.name]
        want = w[v.name] - lr_t * ((1 - b1) * gr) / (np.sqrt((1 - b2) * gr * gr) + eps)
        assert_close(v.numpy(), want, 5e-5, f"Adam step {v.name}")


def test_token_reps_refuse_post_process_and_unequal_lengths():
    from polus_amd.ir.models import TokenReps
    from polus_amd.ir.training import ContrastiveLoss, EfficientDenseRetrievalTrainer, MaxSimScores

    class _M:
        trainable_weights = []

        def query_projection(self, rep, training=False):
            return rep

        def document_projection(self, rep, training=False):
            return rep
    t = EfficientDenseRetrievalTrainer.__new__(EfficientDenseRetrievalTrainer)
    t.model, t.compute_scores, t.post_process_logits = _M(), MaxSimScores(), None
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    m = lambda *s: torch.ones(s, dtype=torch.int32, device="cuda")
    q, d = TokenReps(z(2, 3, 32), m(2, 3)), TokenReps(z(2, 5, 32), m(2, 5))
    with pytest.raises(ValueError):
        t.forward_with_grads(q, d, TokenReps(z(1, 2, 6, 32), m(1, 2, 6)))
    t.post_process_logits = lambda x: x
    with pytest.raises(ValueError):
        t.forward_with_grads(q, d)
