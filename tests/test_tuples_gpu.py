"""GPU: tuple scoring and the distillation losses (polus_amd/csrc/tuples.hip) and their way through the two retrieval
trainers.  MaxSim tuples are held bit for bit to the all-pairs kernels (ops.maxsim_fwd / ops.maxsim_bwd) and, like them,
to the float64 reference at tests/maxsim_cases.TOL; dot tuples and the losses to the float64 references of
tests/tuple_ref.py at the tolerances of tests/tuple_cases.py.  Every check prints its figure before it asserts."""
import functools

import numpy as np
import pytest
import torch

from tests import maxsim_ref
from tests import tuple_cases as tc
from tests import tuple_ref as tr
from tests.maxsim_cases import TOL as MS_TOL
from tests.util import assert_close, host, relerr, rounded

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
NAN = float("nan")


def _dev(a, dtype=None):
    if a is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda()


def _ids(s):
    return "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


@functools.lru_cache(maxsize=None)
def _case(shape, masks):
    return tc.tuple_case(shape, masks)


@functools.lru_cache(maxsize=None)
def _case_ref(shape, masks, mode, layout):
    q, d, qm, dm = _case(shape, masks)
    return tr.maxsim_tuples_fwd(rounded(q, DT[mode]), rounded(d, DT[mode]), qm, dm, layout)


def _tuples_fwd(qt, dt, qm, dm, B, n, Lq, layout, score=None):
    from polus_amd import ops
    score = torch.full((B, n), NAN, dtype=torch.float32, device="cuda") if score is None else score
    am = torch.full((B, n, Lq), 12345, dtype=torch.int32, device="cuda")
    ops.maxsim_tuples_fwd(qt, dt, qm, dm, score, am, layout)
    return score, am


def _tuples_bwd(qt, dt, ds, am, layout):
    from polus_amd import ops
    dq, dd = torch.full_like(qt, NAN), torch.full_like(dt, NAN)
    ops.maxsim_tuples_bwd(qt, dt, ds, am, dq, dd, layout)
    return dq, dd


# ---------------------------------------------------------------------------------------------- 1, 2: MaxSim tuples
@pytest.mark.parametrize("layout", tc.LAYOUTS)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("masks", tc.MASKS)
@pytest.mark.parametrize("shape", tc.SHAPES, ids=_ids)
def test_maxsim_tuples_match_the_all_pairs_kernels_and_the_reference(shape, masks, mode, layout):
    from polus_amd import ops
    B, n, Lq, Ld, E = shape
    N = B * n
    q, d, qm, dm = _case(shape, masks)
    qt, dt, qmt, dmt = _dev(q, DT[mode]), _dev(d, DT[mode]), _dev(qm), _dev(dm)
    rows = tr.doc_rows(B, n, layout)
    rows_t, b_t = torch.as_tensor(rows).cuda(), torch.arange(B, device="cuda")[:, None]
    # forward against the existing kernel: the same bits
    full = torch.full((B, N), NAN, dtype=torch.float32, device="cuda")
    full_am = torch.full((B, N, Lq), 12345, dtype=torch.int32, device="cuda")
    ops.maxsim_fwd(qt, dt, qmt, dmt, full, full_am)
    score, am = _tuples_fwd(qt, dt, qmt, dmt, B, n, Lq, layout)
    torch.cuda.synchronize()
    assert torch.equal(score, full[b_t, rows_t]), "scores differ from polus_maxsim_fwd's"
    assert torch.equal(am, full_am[b_t, rows_t]), "argmax differs from polus_maxsim_fwd's"
    # ... and against the float64 reference
    s_ref, am_ref = _case_ref(shape, masks, mode, layout)
    got, amg = host(score), am.cpu().numpy()
    print(f"[tuples] {shape} {masks} {mode} layout {layout}: score rel err {relerr(got, s_ref):.3e}")
    assert np.isfinite(got).all()
    assert_close(got, s_ref, MS_TOL[mode]["score"], "score")
    assert np.array_equal(amg < 0, am_ref < 0), "-1 exactly where the reference has it"
    assert ((amg >= -1) & (amg < Ld)).all()
    if dm is not None:                                              # never a masked document token
        r_idx = np.broadcast_to(rows[:, :, None], amg.shape)
        assert (dm[r_idx[amg >= 0], amg[amg >= 0]] != 0).all()
    # backward against the existing kernel fed the scattered dscore and the all-pairs argmax
    ds = np.random.Generator(np.random.PCG64(5)).standard_normal((B, n)).astype(np.float32)
    dst = _dev(ds)
    wide = torch.zeros((B, N), dtype=torch.float32, device="cuda")
    wide[b_t, rows_t] = dst
    dq_all, dd_all = torch.full_like(qt, NAN), torch.full_like(dt, NAN)
    ops.maxsim_bwd(qt, dt, wide, full_am, dq_all, dd_all)
    dq, dd = _tuples_bwd(qt, dt, dst, am, layout)
    torch.cuda.synchronize()
    assert torch.equal(dq, dq_all), "dQ differs from polus_maxsim_bwd's"
    assert torch.equal(dd, dd_all), "dD differs from polus_maxsim_bwd's"
    dq_ref, dd_ref = tr.maxsim_tuples_bwd(rounded(q, DT[mode]), rounded(d, DT[mode]), ds, amg, layout)
    dqh, ddh = host(dq), host(dd)
    print(f"[tuples] {shape} {masks} {mode} layout {layout}: dQ rel err {relerr(dqh, dq_ref):.3e}, dD {relerr(ddh, dd_ref):.3e}")
    assert np.isfinite(dqh).all() and np.isfinite(ddh).all(), "an element was not written"
    assert_close(dqh, dq_ref, MS_TOL[mode]["grad"], "dQ")
    assert_close(ddh, dd_ref, MS_TOL[mode]["grad"], "dD")
    if qm is not None:
        assert (dqh[qm == 0] == 0).all(), "masked query rows of dQ must be exactly 0"
    if dm is not None:
        assert (ddh[dm == 0] == 0).all(), "masked document rows of dD must be exactly 0"


# ---------------------------------------------------------------------------------------------- 3: exactness, ties
@pytest.mark.parametrize("layout", tc.LAYOUTS)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_maxsim_tuples_exact_small_integers_and_lowest_j_ties(mode, layout):
    """Integer data: every dot product and score is exact in both engines, so scores and argmax equal the reference
    bit for bit, ties included (the recipe of tests/test_maxsim_gpu.py)."""
    r = np.random.Generator(np.random.PCG64(9))
    B, n, Lq, Ld, E = 2, 2, 20, 40, 64
    N = B * n
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
    rows = tr.doc_rows(B, n, layout)
    for qmask, dmask in ((None, None), (qm, dm)):
        score, am = _tuples_fwd(_dev(q, DT[mode]), _dev(d, DT[mode]), _dev(qmask), _dev(dmask), B, n, Lq, layout)
        torch.cuda.synchronize()
        s_ref, am_ref = tr.maxsim_tuples_fwd(q, d, qmask, dmask, layout)
        amg = am.cpu().numpy()
        assert np.array_equal(score.cpu().numpy(), s_ref.astype(np.float32)), "scores must be exact"
        assert np.array_equal(amg, am_ref)
        zero = amg[rows == 2]                                       # the pair with the all-zero document
        assert (zero[zero >= 0] == 0).all() and (zero >= 0).any()
        assert not np.isin(amg, [25, 33]).any(), "a duplicate won over token 7"


# ---------------------------------------------------------------------------------------------- 4: strides, determinism
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_maxsim_tuples_strided_destination_and_determinism(mode):
    shape, layout = (5, 4, 33, 180, 128), 0
    B, n, Lq, Ld, E = shape
    q, d, qm, dm = _case(shape, "ragged")
    qt, dt, qmt, dmt = _dev(q, DT[mode]), _dev(d, DT[mode]), _dev(qm), _dev(dm)
    big = torch.full((B, 3 * n + 5), -7.25, dtype=torch.float32, device="cuda")
    _, am = _tuples_fwd(qt, dt, qmt, dmt, B, n, Lq, layout, score=big[:, n:2 * n])
    score, am2 = _tuples_fwd(qt, dt, qmt, dmt, B, n, Lq, layout)
    torch.cuda.synchronize()
    bh = big.cpu().numpy()
    assert (bh[:, :n] == -7.25).all() and (bh[:, 2 * n:] == -7.25).all(), "columns outside the block were written"
    assert torch.equal(big[:, n:2 * n], score) and torch.equal(am, am2)
    ds = _dev(np.random.Generator(np.random.PCG64(3)).standard_normal((B, n)).astype(np.float32))
    wide = torch.zeros((B, 2 * n + 1), dtype=torch.float32, device="cuda")
    wide[:, 1:n + 1] = ds
    dq1, dd1 = _tuples_bwd(qt, dt, ds, am, layout)
    dq2, dd2 = _tuples_bwd(qt, dt, ds, am, layout)
    dq3, dd3 = _tuples_bwd(qt, dt, wide[:, 1:n + 1], am, layout)    # strided dscore
    torch.cuda.synchronize()
    for a, b in ((dq1, dq2), (dd1, dd2), (dq1, dq3), (dd1, dd3)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- 5: dot tuples
def _framed(a, ld, off, dtype):
    """A [rows, W] view with row stride ld, `off` elements into a NaN-poisoned buffer, holding `a` (None: left poisoned)."""
    rows, W = a.shape if hasattr(a, "shape") else a
    flat = torch.full((off + rows * ld + 8,), NAN, dtype=dtype, device="cuda")
    v = flat[off:].as_strided((rows, W), (ld, 1))
    if hasattr(a, "shape"):
        v.copy_(_dev(a, dtype))
    return flat, v


def _dot_run(q, d, ds, mode, layout, aligned):
    """Scores and gradients with every operand 16-byte aligned with strides of whole chunks, or none of them."""
    from polus_amd import ops
    B, W = q.shape
    N = d.shape[0]
    n = N // B
    ld = (W + 7) // 8 * 8 + (8 if aligned else 3)
    off = 0 if aligned else 1
    dt = DT[mode]
    _, qv = _framed(q, ld, off, dt)
    _, dv = _framed(d, ld, off, dt)
    sflat, score = _framed((B, n), n + 2, 1, torch.float32)
    ops.dot_tuples_fwd(qv, dv, score, layout)
    dqf, dq = _framed((B, W), ld, off, dt)
    ddf, dd = _framed((N, W), ld, off, dt)
    wide = torch.zeros((B, n + 3), dtype=torch.float32, device="cuda")
    wide[:, 2:n + 2] = _dev(ds)
    ops.dot_tuples_bwd(qv, dv, wide[:, 2:n + 2], dq, dd, layout)
    torch.cuda.synchronize()
    for flat, view in ((sflat, score), (dqf, dq), (ddf, dd)):      # nothing outside the views was written
        probe = flat.clone()
        probe[view.storage_offset():].as_strided(tuple(view.shape), view.stride()).fill_(NAN)
        assert probe.isnan().all(), "a dot-tuples kernel wrote outside its output"
    return score.clone(), dq.clone(), dd.clone()


@pytest.mark.parametrize("layout", tc.LAYOUTS)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("W", tc.DOT_W)
def test_dot_tuples_match_the_reference_with_both_access_widths(W, mode, layout):
    q, d, ds = tc.dot_case(W)
    qr, dr = rounded(q, DT[mode]), rounded(d, DT[mode])
    tol = tc.TOL["dot_" + mode]
    s_ref = tr.dot_tuples_fwd(qr, dr, layout)
    dq_ref, dd_ref = tr.dot_tuples_bwd(qr, dr, ds, layout)
    outs = []
    for aligned in (True, False):
        score, dq, dd = _dot_run(q, d, ds, mode, layout, aligned)
        es, eq, ed = relerr(host(score), s_ref), relerr(host(dq), dq_ref), relerr(host(dd), dd_ref)
        print(f"[tuples] dot W={W} {mode} layout {layout} aligned={aligned}: score {es:.3e} dq {eq:.3e} dd {ed:.3e}")
        assert torch.isfinite(score).all() and torch.isfinite(dq.float()).all() and torch.isfinite(dd.float()).all()
        assert es <= tol["score"] and eq <= tol["grad"] and ed <= tol["grad"]
        outs.append((score, dq, dd))
    for a, b in zip(*outs):
        assert torch.equal(a, b), "16-byte and single-element accesses must give the same bits"


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_dot_tuples_exact_on_small_integers(mode):
    r = np.random.Generator(np.random.PCG64(11))
    B, n, W = 3, 4, 1000
    q = r.integers(-3, 4, size=(B, W)).astype(np.float32)
    d = r.integers(-3, 4, size=(B * n, W)).astype(np.float32)
    ds = r.integers(-2, 3, size=(B, n)).astype(np.float32)
    for layout in tc.LAYOUTS:
        score, dq, dd = _dot_run(q, d, ds, mode, layout, True)
        dq_ref, dd_ref = tr.dot_tuples_bwd(q, d, ds, layout)
        assert np.array_equal(host(score), tr.dot_tuples_fwd(q, d, layout))
        assert np.array_equal(host(dq), dq_ref) and np.array_equal(host(dd), dd_ref)


# ---------------------------------------------------------------------------------------------- 6: losses
def _loss_run(kind, s, t, strided):
    from polus_amd import ops
    rows, n = s.shape
    fn = ops.distill_kl if kind == "kl" else ops.margin_mse
    if strided:
        _, sv = _framed(s, n + 3, 1, torch.float32)
        _, tv = _framed(t, n + 5, 2, torch.float32)
        gflat, g = _framed((rows, n), n + 1, 3, torch.float32)
    else:
        sv, tv = _dev(s), _dev(t)
        gflat = torch.full((rows * n,), NAN, dtype=torch.float32, device="cuda")
        g = gflat.view(rows, n)
    loss = torch.full((1,), NAN, dtype=torch.float32, device="cuda")
    fn(sv, tv, loss, g)
    torch.cuda.synchronize()
    probe = gflat.clone()
    probe[g.storage_offset():].as_strided(tuple(g.shape), g.stride()).fill_(NAN)
    assert probe.isnan().all(), "the loss kernel wrote outside dstudent"
    return loss.clone(), g.clone()


@pytest.mark.parametrize("kind", ["kl", "mse"])
@pytest.mark.parametrize("shape", tc.LOSS_SHAPES, ids=_ids)
def test_distillation_losses_match_the_reference(shape, kind):
    rows, n = shape
    s, t = tc.loss_case(rows, n, kind)
    loss_ref, g_ref = (tr.distill_kl if kind == "kl" else tr.margin_mse)(s, t)
    tol = tc.TOL[kind]
    loss, g = _loss_run(kind, s, t, strided=False)
    loss2, g2 = _loss_run(kind, s, t, strided=False)
    loss3, g3 = _loss_run(kind, s, t, strided=True)
    el, eg = relerr(host(loss)[0], loss_ref), relerr(host(g), g_ref)
    print(f"[tuples] {kind} {rows}x{n}: loss {float(loss):.6f} (reference {loss_ref:.6f}) rel err {el:.3e}, gradient {eg:.3e}")
    assert torch.isfinite(loss).all() and torch.isfinite(g).all(), "not fully written, or an absent column's student value was used"
    assert el <= tol["loss"] and eg <= tol["grad"]
    gh = g.cpu().numpy()
    assert (gh[np.isneginf(t)] == 0).all(), "absent columns get exactly zero gradient"
    if rows >= 3:
        assert (gh[1] == 0).all(), "the all-absent row"
    if kind == "mse" and rows >= 5:
        assert (gh[2] == 0).all(), "the row without a positive"
    for a, b in ((loss, loss2), (g, g2), (loss, loss3), (g, g3)):
        assert torch.equal(a, b), "two runs (and strided operands) must give the same bits"


# ---------------------------------------------------------------------------------------------- 7: trainer steps
def _dense_setup(mode, k, scorer, loss):
    """The construction of tests/test_maxsim_gpu.py::test_late_interaction_trainer_step: two frozen BERT encoders of
    the committed golden, ragged masks, k explicit negatives."""
    from polus_amd.ir.models import LateInteractionDualEncoder
    from polus_amd.ir.training import EfficientDenseRetrievalTrainer
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

    def batch(S, shape):
        ids = r.integers(1, ocfg.vocab_size, size=shape + (S,)).astype(np.int32)
        lens = r.integers(1, S + 1, size=shape)
        return {"input_ids": ids, "attention_mask": (np.arange(S) < lens[..., None]).astype(np.int32)}
    q, d, neg = batch(Sq, (B,)), batch(Sd, (B,)), batch(Sd, (B, k))
    model = LateInteractionDualEncoder(qenc, denc, projection_dim=E, compute_dtype=mode)
    trainer = EfficientDenseRetrievalTrainer(model, scorer, optimizer=Adam(1e-3), loss=loss)
    return dict(trainer=trainer, model=model, qenc=qenc, denc=denc, ocfg=ocfg, params=params, q=q, d=d, neg=neg,
                B=B, Sq=Sq, E=E, k=k, w={v.name: v.numpy().astype(np.float64) for v in model.trainable_weights})


def _dense_oracle(c, am, dloss):
    """Projection -> normalise -> tuple MaxSim -> `dloss` (scores -> (loss, dscores)) in float64, backward with the
    device's argmax: (loss, the four projection gradients in the order of model.trainable_weights)."""
    from oracle import bert as ob
    params, ocfg, q, d, neg, k, E = c["params"], c["ocfg"], c["q"], c["d"], c["neg"], c["k"], c["E"]
    names = [v.name for v in c["model"].trainable_weights]
    wq, bq, wd, bd = (c["w"][x] for x in names)
    hq = ob.bert_fwd(params, ocfg, q["input_ids"], q["attention_mask"])[0]
    dids, dmask = [d["input_ids"]], [d["attention_mask"]]
    for i in range(k):
        dids.append(neg["input_ids"][:, i]); dmask.append(neg["attention_mask"][:, i])
    hd = np.concatenate([ob.bert_fwd(params, ocfg, a, m)[0] for a, m in zip(dids, dmask)], 0)
    dm, qm = np.concatenate(dmask, 0), q["attention_mask"]
    pq, pd_ = hq @ wq.T + bq, hd @ wd.T + bd
    yq, _ = maxsim_ref.l2norm_fwd(pq)
    yd, _ = maxsim_ref.l2norm_fwd(pd_)
    s_ref, _ = tr.maxsim_tuples_fwd(yq, yd, qm, dm, 0)
    loss_ref, ds = dloss(s_ref)
    gq, gd = tr.maxsim_tuples_bwd(yq, yd, ds, am, 0)
    dq, dd = maxsim_ref.l2norm_bwd(pq, gq), maxsim_ref.l2norm_bwd(pd_, gd)
    grads = [dq.reshape(-1, E).T @ hq.reshape(-1, hq.shape[-1]), dq.reshape(-1, E).sum(0),
             dd.reshape(-1, E).T @ hd.reshape(-1, hd.shape[-1]), dd.reshape(-1, E).sum(0)]
    return float(loss_ref), dict(zip(names, grads)), qm


def _check_dense_step(c, mode, loss, dloss):
    """Loss and projection gradients against the oracle, the encoders untouched, the first Adam step (the checks and
    the tolerances of test_late_interaction_trainer_step)."""
    B, k, Sq = c["B"], c["k"], c["Sq"]
    am = c["trainer"].compute_scores.argmax.cpu().numpy()
    assert am.shape == (B, 1 + k, Sq)
    loss_ref, g_ref, qm = _dense_oracle(c, am, dloss)
    print(f"[tuples] dense trainer {mode}: loss {loss:.6f} (reference {loss_ref:.6f})")
    assert abs(loss - loss_ref) < (1e-4 if mode == "f32" else 5e-2) * max(1.0, abs(loss_ref)), (loss, loss_ref)
    assert (am[np.broadcast_to(qm[:, None, :] == 0, am.shape)] == -1).all()
    grads = {v.name: v.grad.detach().cpu().numpy().astype(np.float64) for v in c["model"].trainable_weights}
    tol = 5e-4 if mode == "f32" else 8e-2
    for name, want in g_ref.items():
        print(f"[tuples] dense trainer {mode}: {name} rel err {relerr(grads[name], want):.3e}")
        assert_close(grads[name], want, tol, name)
    b1, b2, eps, lr = 0.9, 0.999, 1e-7, 1e-3
    lr_t = lr * np.sqrt(1 - b2) / (1 - b1)
    for v in c["model"].trainable_weights:
        gr = grads[v.name]
        want = c["w"][v.name] - lr_t * ((1 - b1) * gr) / (np.sqrt((1 - b2) * gr * gr) + eps)
        assert_close(v.numpy(), want, 5e-5, f"Adam step {v.name}")


def _teacher(B, k, seed):
    """Seeded teacher scores at the scale of normalised MaxSim over 12 query tokens, one column absent."""
    t = np.random.Generator(np.random.PCG64(seed)).uniform(0.0, 6.0, size=(B, 1 + k)).astype(np.float32)
    t[2, 1] = -np.inf
    return t


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_distillation_trainer_step_late_interaction_kl(mode):
    from polus_amd.ir.models import TokenReps
    from polus_amd.ir.training import DistillKLLoss, TupleMaxSimScores
    c = _dense_setup(mode, 2, TupleMaxSimScores(), DistillKLLoss())
    trainer, teacher = c["trainer"], _teacher(6, 2, 77)
    before = (c["qenc"].arena.params.clone(), c["denc"].arena.params.clone())
    reps = trainer.forward_without_grads(c["q"], c["d"], c["neg"], teacher)
    assert len(reps) == 4 and all(isinstance(x, TokenReps) for x in reps[:3])
    assert reps[3].is_cuda and reps[3].dtype == torch.float32 and tuple(reps[3].shape) == (6, 3)
    loss = float(trainer.train_step(c["q"], c["d"], c["neg"], teacher))
    torch.cuda.synchronize()
    assert torch.equal(before[0], c["qenc"].arena.params) and torch.equal(before[1], c["denc"].arena.params)
    _check_dense_step(c, mode, loss, lambda s: tr.distill_kl(s, teacher))
    dpos, dneg = trainer.loss.backward()
    assert tuple(dpos.shape) == (6, 1) and tuple(dneg.shape) == (6, 2) and float(dneg[2, 0]) == 0.0


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_tuple_contrastive_trainer_step_without_a_teacher(mode):
    from oracle import losses as ol
    from polus_amd.ir.training import TupleContrastiveLoss, TupleMaxSimScores
    c = _dense_setup(mode, 2, TupleMaxSimScores(), TupleContrastiveLoss())
    loss = float(c["trainer"].train_step(c["q"], c["d"], c["neg"]))
    torch.cuda.synchronize()
    _check_dense_step(c, mode, loss, lambda s: ol.sparse_softmax_xent_fwd(s, np.zeros(s.shape[0], np.int64)))


def _sparse_step(scorer, loss, teacher=None, lam=(0.1, 0.05)):
    from tests import test_splade_gpu as tsg
    from polus_amd.ir.training import SparseRetrievalTrainer
    from polus_amd.optimizers import AdamWeightDecay
    model, ocfg, _ = tsg._model("f32")
    model.deterministic = True
    t = SparseRetrievalTrainer(model, AdamWeightDecay(learning_rate=1e-3, weight_decay_rate=0.01), compute_scores=scorer,
                               lambda_q=lam[0], lambda_d=lam[1], loss=loss)
    batch, (ids, mask) = tsg._step_batch(ocfg, 60)
    before = model.arena.params.clone()
    got = float(t.train_step(*batch) if teacher is None else t.train_step(*batch, teacher))
    torch.cuda.synchronize()
    assert t.optimizer.iterations == 1 and not torch.equal(before, model.arena.params)
    from tests import splade_ref as sr
    ref_rep, _ = sr.splade_fwd(tsg._params(), ocfg, ids, mask, None)
    B = 2
    scores = tr.dot_tuples_fwd(ref_rep[:B], ref_rep[B:], 0)
    rq, rd = sr.flops_reg(ref_rep[:B], lam[0])[0], sr.flops_reg(ref_rep[B:], lam[1])[0]
    return got, scores, rq, rd, tsg.TOLS["f32"]["loss"]


def test_distillation_trainer_step_splade_margin_mse():
    from polus_amd.ir.training import MarginMSELoss, TupleDotScores
    teacher = np.array([[1.5, 0.5], [0.5, 1.5]], np.float32)        # margins of the student's order: the loss stays of order 1
    got, scores, rq, rd, tol = _sparse_step(TupleDotScores(), MarginMSELoss(), teacher)
    mse = float(tr.margin_mse(scores, teacher)[0])
    print(f"[tuples] sparse trainer: loss {got:.6f} (reference {mse + rq + rd:.6f} = {mse:.6f} + {rq:.6f} + {rd:.6f})")
    assert abs(got - (mse + rq + rd)) < tol
    assert rq > 100 * tol and rd > 100 * tol and mse > 100 * tol


def test_tuple_contrastive_trainer_step_splade_without_a_teacher():
    from oracle import losses as ol
    from polus_amd.ir.training import TupleContrastiveLoss, TupleDotScores
    got, scores, rq, rd, tol = _sparse_step(TupleDotScores(), TupleContrastiveLoss())
    con = float(ol.sparse_softmax_xent_fwd(scores, np.zeros(2, np.int64))[0])
    print(f"[tuples] sparse trainer, contrastive: loss {got:.6f} (reference {con + rq + rd:.6f})")
    assert abs(got - (con + rq + rd)) < tol


def test_teacher_scores_replay_in_the_step_graph():
    """A `teacher_scores` leaf of the batch (host here) is copied into a static tensor like every other leaf: the
    replayed steps, each with its own batch and teacher scores, give the bits of eager steps."""
    from tests import test_splade_gpu as tsg
    from polus_amd.ir.training import MarginMSELoss, SparseRetrievalTrainer, TupleDotScores
    from polus_amd.optimizers import AdamWeightDecay

    def train(graph):
        model, ocfg, _ = tsg._model("f32")
        model.deterministic = True
        t = SparseRetrievalTrainer(model, AdamWeightDecay(learning_rate=1e-3, weight_decay_rate=0.01),
                                   compute_scores=TupleDotScores(), lambda_q=0.1, lambda_d=0.05, loss=MarginMSELoss())
        if graph:
            t.enable_step_graph(warmup=1)
        losses = []
        for s in range(3):
            batch, _ = tsg._step_batch(ocfg, 60 + s)
            teacher = np.random.Generator(np.random.PCG64(s)).uniform(0, 3, size=(2, 2)).astype(np.float32)
            losses.append(float(t.train_step(*batch, teacher)))
        torch.cuda.synchronize()
        return t, losses, model.arena.params.clone()
    _, eager, params = train(False)
    tg, replayed, params_g = train(True)
    assert tg._graphed.graph is not None, "the step was not captured"
    assert len(set(eager)) == 3, "the steps must differ for the comparison to mean anything"
    assert eager == replayed and torch.equal(params, params_g), "the replayed step graph differs from eager steps"


def test_a_batch_without_teacher_scores_takes_the_old_path_to_the_same_bits():
    """MaxSimScores + ContrastiveLoss: the same step with the batch as it always was and with the new optional
    element passed as None."""
    from polus_amd.ir.training import ContrastiveLoss, MaxSimScores
    out = []
    for extra in ((), (None,)):
        c = _dense_setup("bf16", 2, MaxSimScores(), ContrastiveLoss())
        reps = c["trainer"].forward_without_grads(c["q"], c["d"], c["neg"], *extra)
        assert len(reps) == 3
        loss = c["trainer"].train_step(c["q"], c["d"], c["neg"], *extra)
        torch.cuda.synchronize()
        assert tuple(c["trainer"].compute_scores.scores.shape) == (6, 18)
        out.append((loss.t.clone(), c["model"].arena.grads.clone(), c["model"].arena.params.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- 8: refusals
def _refused(fn, msg):
    from polus_amd._lib import PolusHipError
    with pytest.raises(PolusHipError) as e:
        fn()
    assert msg in str(e.value), str(e.value)


def test_refusals_name_their_limit():
    """Device tensors of the invalid shapes, sized for the call they make: a refusal that did not fire would still
    launch on valid memory."""
    from polus_amd import ops
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device="cuda")
    e = lambda *s, dtype=torch.float32: torch.empty(s, dtype=dtype, device="cuda")

    def call(B, n, Lq, Ld, E, layout=0):
        q, d, s, am = z(B, Lq, E), z(B * n, Ld, E), e(B, n), e(B, n, Lq, dtype=torch.int32)
        return (lambda: ops.maxsim_tuples_fwd(q, d, None, None, s, am, layout),
                lambda: ops.maxsim_tuples_bwd(q, d, s, am, torch.empty_like(q), torch.empty_like(d), layout))

    for args, msg in (((1, 1, 1, 1, 48), "multiple of 32"), ((1, 1, 1, 1, 288), "multiple of 32"),
                      ((1, 1, 513, 1, 32), "Lq <= 512"), ((1, 1, 1, 513, 32), "Ld <= 512"),
                      ((65536, 1, 1, 1, 32), "B <= 65535"), ((1, 65536, 1, 1, 32), "n <= 65535"),
                      ((2, 2, 4, 4, 32, 2), "layout")):
        f, b = call(*args)
        _refused(f, msg)
        _refused(b, msg)
    # B*n*Lq = 2^31: the argmax alone is 8.6 GB, allocated but never written
    f, b = call(4096, 1024, 512, 1, 32)
    _refused(f, "2^31")
    _refused(b, "2^31")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    _refused(lambda: ops.dot_tuples_fwd(z(65536, 1), z(65536, 1), e(65536, 1)), "B <= 65535")
    _refused(lambda: ops.dot_tuples_fwd(z(1, 1), z(65536, 1), e(1, 65536)), "n <= 65535")
    _refused(lambda: ops.dot_tuples_fwd(z(2, 0), z(4, 0), e(2, 2)), "W >= 1")
    _refused(lambda: ops.dot_tuples_bwd(z(2, 4), z(4, 4), z(2, 2), e(2, 4), e(4, 4), 3), "layout")
    for fn in (ops.distill_kl, ops.margin_mse):
        _refused(lambda: fn(z(2, 1025), z(2, 1025), e(1), e(2, 1025)), "n <= 1024")
        _refused(lambda: fn(z(0, 4), z(0, 4), e(1), e(0, 4)), "rows >= 1")
    torch.cuda.synchronize()


def test_cpu_tensors_are_refused():
    from polus_amd import ops
    from polus_amd._lib import PolusHipError
    q, s, am = torch.zeros((1, 1, 32)), torch.zeros(1, 1), torch.zeros(1, 1, 1, dtype=torch.int32)
    v = torch.zeros(1, 4)
    for fn in (lambda: ops.maxsim_tuples_fwd(q, q, None, None, s, am), lambda: ops.maxsim_tuples_bwd(q, q, s, am, q.clone(), q.clone()),
               lambda: ops.dot_tuples_fwd(v, v, s), lambda: ops.dot_tuples_bwd(v, v, s, v.clone(), v.clone()),
               lambda: ops.distill_kl(v, v, torch.zeros(1), v.clone()), lambda: ops.margin_mse(v, v, torch.zeros(1), v.clone())):
        with pytest.raises(PolusHipError):
            fn()


def test_scorers_need_negatives_and_teacher_scores_their_shape():
    from polus_amd.ir.models import TokenReps
    from polus_amd.ir.training import (DistillKLLoss, EfficientDenseRetrievalTrainer, MarginMSELoss, SparseRetrievalTrainer,
                                       TupleDotScores, TupleMaxSimScores)
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    m = lambda *s: torch.ones(s, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="negatives"):
        TupleMaxSimScores()(TokenReps(z(2, 3, 32), m(2, 3)), TokenReps(z(2, 5, 32), m(2, 5)))
    with pytest.raises(ValueError, match="negatives"):
        TupleDotScores()(z(2, 8), z(2, 8))

    class _Launched:
        """A model that must not be reached: the shape check comes before any launch."""
        trainable_weights = []

        def __getattr__(self, name):
            raise AssertionError(f"model.{name} was reached before teacher_scores were checked")

        def __call__(self, *a, **kw):
            raise AssertionError("the model ran before teacher_scores were checked")
    ids = lambda *s: {"input_ids": np.ones(s, np.int32), "attention_mask": np.ones(s, np.int32)}
    for cls, method in ((EfficientDenseRetrievalTrainer, "forward_without_grads"), (SparseRetrievalTrainer, "forward_with_grads")):
        t = cls.__new__(cls)
        t.model, t.compute_scores, t.post_process_logits = _Launched(), TupleDotScores(), None
        for bad in (np.zeros((2, 2), np.float32), np.zeros((3, 3), np.float32), np.zeros(6, np.float32), z(2, 4)):
            with pytest.raises(ValueError, match="teacher_scores"):
                getattr(t, method)(ids(2, 8), ids(2, 8), ids(2, 2, 8), bad)
        with pytest.raises(ValueError, match="negatives"):
            getattr(t, method)(ids(2, 8), ids(2, 8), None, np.zeros((2, 1), np.float32))
    for loss in (DistillKLLoss(), MarginMSELoss()):
        s = z(2, 3)
        with pytest.raises(ValueError, match="teacher_scores"):
            loss(s[:, :1], s[:, 1:], np.zeros((2, 2), np.float32))
