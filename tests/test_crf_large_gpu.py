"""GPU: the linear-chain CRF for 17 <= C <= 128 tags (polus_amd/csrc/crf.hip, one workgroup per sequence)
against the NumPy oracle -- kernel parity (ragged lengths, f32 / bf16 dpot, sample weights, accumulate),
BIO-masked transitions, exact Viterbi, run-to-run determinism, and the NER models end to end."""
import numpy as np
import pytest
import torch

from oracle import bert as ob
from oracle import losses as ol
from tests.util import assert_close, dev, host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from polus_amd import ops as _ops
    return _ops


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def ragged_lengths(r, B, S):
    L = r.integers(1, S + 1, size=B).astype(np.int32)
    L[0] = S
    if B > 2:
        L[1] = 0
        L[2] = 1
    return L


def bio_mask(n_types):
    """PAD, O, then B-X / I-X for each type: I-X may only follow B-X or I-X."""
    C = 2 + 2 * n_types
    m = np.ones((C, C), np.float32)
    for i in range(n_types):
        ix = 3 + 2 * i
        m[:, ix] = 0
        m[ix - 1, ix] = m[ix, ix] = 1
    return m


def run_nll(ops, pot, tags, lengths, trans, weights, dtype, dtrans0=None):
    B, S, C = pot.shape
    loss = torch.empty(1, device="cuda")
    dpot = torch.full((B, S, C), float("nan"), device="cuda", dtype=dtype)
    dT = dev(dtrans0) if dtrans0 is not None else torch.full((C, C), float("nan"), device="cuda")
    ops.crf_nll(dev(pot), dev(tags), dev(lengths), dev(trans), None if weights is None else dev(weights), loss, dpot, dT,
                accumulate=dtrans0 is not None)
    return float(loss), host(dpot), host(dT)


@pytest.mark.parametrize("B,S,C", [(5, 40, 17), (4, 64, 32), (3, 96, 64), (2, 128, 128), (8, 33, 100)])
def test_crf_large_matches_oracle(ops, B, S, C):
    r = rng(B * 1000 + S + C)
    pot = (r.standard_normal((B, S, C)) * 2).astype(np.float32)
    tags = r.integers(0, C, size=(B, S)).astype(np.int32)
    lengths = ragged_lengths(r, B, S)
    trans = (r.standard_normal((C, C)) * 0.5).astype(np.float32)
    onehot = np.eye(C)[tags]
    sw = r.uniform(0.5, 1.5, size=B).astype(np.float32)
    for weights in (None, sw):
        loss_ref, dx_ref, dT_ref = ol.crf_nll_fwd(onehot, pot, lengths, trans, None, weights)
        loss, dpot, dT = run_nll(ops, pot, tags, lengths, trans, weights, torch.float32)
        assert abs(loss - loss_ref) < 2e-5 * max(1, abs(loss_ref))
        assert_close(dpot, dx_ref, 1e-4, "crf dpot")
        assert_close(dT, dT_ref, 2e-4, "crf dtrans")
        for b in range(B):
            assert not dpot[b, lengths[b]:].any()                  # rows >= L are zero (all rows at L = 0)
        # bf16 dpot: the f32 gradient rounded once
        _, dpot16, dT16 = run_nll(ops, pot, tags, lengths, trans, weights, torch.bfloat16)
        assert_close(dpot16, dx_ref, 5e-3, "crf dpot bf16")     # bf16 rounding: <= 2^-9 relative per element
        assert np.array_equal(dT16, dT)
    # accumulate onto a pre-filled dtrans
    d0 = r.standard_normal((C, C)).astype(np.float32)
    loss_ref, _, dT_ref = ol.crf_nll_fwd(onehot, pot, lengths, trans, None, sw)
    _, _, dT = run_nll(ops, pot, tags, lengths, trans, sw, torch.float32, dtrans0=d0)
    assert_close(dT - d0, dT_ref, 2e-4, "crf dtrans accumulate")


def test_crf_large_bio_masked_transitions(ops):
    n_types = 20
    mask = bio_mask(n_types)
    C = mask.shape[0]
    B, S = 6, 80
    r = rng(42)
    pot = (r.standard_normal((B, S, C)) * 2).astype(np.float32)
    tags = r.integers(1, C, size=(B, S)).astype(np.int32)
    for b in range(B):                                          # gold paths obey the mask
        for s in range(S):
            t = tags[b, s]
            if t >= 3 and t % 2 == 1 and (s == 0 or tags[b, s - 1] not in (t - 1, t)):
                tags[b, s] = t - 1
    lengths = ragged_lengths(r, B, S)
    trans = (r.standard_normal((C, C)) * 0.5).astype(np.float32)
    onehot = np.eye(C)[tags]
    masked = ol.crf_transitions(trans, mask)
    loss_ref, dx_ref, dT_ref = ol.crf_nll_fwd(onehot, pot, lengths, trans, mask, None)
    loss, dpot, dT = run_nll(ops, pot, tags, lengths, masked, None, torch.float32)
    dT = dT * mask
    assert abs(loss - loss_ref) < 2e-5 * max(1, abs(loss_ref))
    assert_close(dpot, dx_ref, 1e-4, "masked crf dpot")
    assert_close(dT, dT_ref, 2e-4, "masked crf dtrans")
    assert np.isfinite(dT).all()
    # an all-masked column (every entry -10000) stays finite
    m2 = mask.copy()
    m2[:, 5] = 0
    loss_ref, dx_ref, dT_ref = ol.crf_nll_fwd(np.eye(C)[np.where(tags == 5, 4, tags)], pot, lengths, trans, m2, None)
    loss, dpot, dT = run_nll(ops, pot, np.where(tags == 5, 4, tags).astype(np.int32), lengths,
                             ol.crf_transitions(trans, m2), None, torch.float32)
    assert abs(loss - loss_ref) < 2e-5 * max(1, abs(loss_ref))
    assert_close(dpot, dx_ref, 1e-4, "all-masked column dpot")
    assert_close(dT * m2, dT_ref, 2e-4, "all-masked column dtrans")
    # Viterbi never takes a masked transition
    dec = torch.empty((B, S), dtype=torch.int32, device="cuda")
    ops.crf_viterbi(dev(pot), dev(lengths), dev(masked), dec)
    dec = dec.cpu().numpy()
    ref = ol.crf_viterbi(pot, lengths, masked)
    for b in range(B):
        L = lengths[b]
        assert all(mask[dec[b, s - 1], dec[b, s]] for s in range(1, L))
        if L:
            best = path_score(pot[b], masked, ref[b], L)
            assert abs(path_score(pot[b], masked, dec[b], L) - best) <= 1e-5 * max(1.0, abs(best))


def path_score(pot, trans, path, L):
    x, T = pot.astype(np.float64), trans.astype(np.float64)
    return x[np.arange(L), path[:L]].sum() + T[path[:L - 1], path[1:L]].sum()


@pytest.mark.parametrize("B,S,C", [(5, 40, 17), (4, 64, 32), (3, 96, 64), (2, 128, 128), (8, 33, 100)])
def test_crf_large_viterbi(ops, B, S, C):
    r = rng(7 * B + S + C)
    lengths = ragged_lengths(r, B, S)
    # dyadic grid: every path sum exact in f32 and float64, ties decided by the same rule
    pot = (r.integers(-64, 65, size=(B, S, C)) / 16.0).astype(np.float32)
    trans = (r.integers(-8, 9, size=(C, C)) / 16.0).astype(np.float32)
    pot[:, :, C - 3:] = pot[:, :, :3]                             # duplicate tags: deliberate ties
    trans[C - 3:, :] = trans[:3, :]
    trans[:, C - 3:] = trans[:, :3]
    dec = torch.empty((B, S), dtype=torch.int32, device="cuda")
    ops.crf_viterbi(dev(pot), dev(lengths), dev(trans), dec)
    assert np.array_equal(dec.cpu().numpy(), ol.crf_viterbi(pot, lengths, trans))
    # random normals: the decoded path scores as the best one
    pot = r.standard_normal((B, S, C)).astype(np.float32)
    trans = (r.standard_normal((C, C)) * 0.5).astype(np.float32)
    dec = torch.full((B, S), -1, dtype=torch.int32, device="cuda")
    ops.crf_viterbi(dev(pot), dev(lengths), dev(trans), dec)
    got = dec.cpu().numpy()
    ref = ol.crf_viterbi(pot, lengths, trans)
    for b in range(B):
        L = lengths[b]
        assert not got[b, L:].any()
        if L:
            best = path_score(pot[b], trans, ref[b], L)
            assert abs(path_score(pot[b], trans, got[b], L) - best) <= 1e-5 * max(1.0, abs(best))


def test_crf_large_deterministic(ops):
    B, S, C = 64, 256, 128
    r = rng(5)
    pot = (r.standard_normal((B, S, C)) * 2).astype(np.float32)
    tags = r.integers(0, C, size=(B, S)).astype(np.int32)
    lengths = r.integers(S // 2, S + 1, size=B).astype(np.int32)
    trans = (r.standard_normal((C, C)) * 0.5).astype(np.float32)
    sw = r.uniform(0.5, 1.5, size=B).astype(np.float32)
    outs = []
    for _ in range(2):
        loss = torch.empty(1, device="cuda")
        dpot = torch.empty((B, S, C), device="cuda")
        dT = torch.empty((C, C), device="cuda")
        ops.crf_nll(dev(pot), dev(tags), dev(lengths), dev(trans), dev(sw), loss, dpot, dT)
        dec = torch.empty((B, S), dtype=torch.int32, device="cuda")
        ops.crf_viterbi(dev(pot), dev(lengths), dev(trans), dec)
        outs.append([loss.cpu().numpy(), dpot.cpu().numpy(), dT.cpu().numpy(), dec.cpu().numpy()])
    for a, b in zip(*outs):
        assert np.isfinite(a.astype(np.float64)).all() and np.array_equal(a, b)
    assert np.isfinite(float(outs[0][0][0]))


def test_crf_more_than_128_tags_refused(ops):
    from polus_amd._lib import PolusHipError
    B, S, C = 2, 4, 129
    pot = torch.zeros((B, S, C), device="cuda")
    tags = torch.zeros((B, S), dtype=torch.int32, device="cuda")
    L = torch.full((B,), S, dtype=torch.int32, device="cuda")
    T = torch.zeros((C, C), device="cuda")
    with pytest.raises(PolusHipError, match="128"):
        ops.crf_nll(pot, tags, L, T, None, torch.empty(1, device="cuda"), torch.empty_like(pot), torch.empty_like(T))
    with pytest.raises(PolusHipError, match="128"):
        ops.crf_viterbi(pot, L, T, torch.empty((B, S), dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------------------ models
def _ner_inputs(seed, B, S, C):
    r = rng(seed)
    x = r.standard_normal((B, S, 768)).astype(np.float32)
    tags = r.integers(0, C, size=(B, S))
    return x, np.eye(C, dtype=np.float32)[tags]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_ner_mlp_crf_25_tags_step_matches_oracle(mode):
    """baselineNER_MLP_CRF(output_classes=25): loss, every gradient and the decode against the oracle.  f32: the
    whole head in float64; bf16: the CRF part on the engine's own potentials (the Dense layers run in bf16)."""
    from polus_amd.ner.models import baselineNER_MLP_CRF
    B, S, C = 4, 24, 25
    x, y = _ner_inputs(9, B, S, C)
    model = baselineNER_MLP_CRF(sequence_length=S, output_classes=C, compute_dtype=mode)
    n = [v.name for v in model.trainable_weights]
    w = {v.name: v.numpy().astype(np.float64) for v in model.trainable_weights}
    pot = model(x, training=True)
    assert pot.shape == (B, S, C) and pot.dtype == torch.float32
    if mode == "f32":
        u = x.reshape(-1, 768).astype(np.float64) @ w[n[0]].T + w[n[1]]
        hdn = ob.swish(u)
        pot_ref = (hdn @ w[n[2]].T + w[n[3]]).reshape(B, S, C)
        assert_close(host(pot), pot_ref, 1e-4, "potentials")
    else:
        pot_ref = host(pot)
    loss = float(model.loss(y, pot))
    loss_ref, dpot, dT = ol.crf_nll_fwd(y, pot_ref, np.full(B, S), w[n[4]])
    assert abs(loss - loss_ref) < 1e-4 * max(1.0, abs(loss_ref))
    loss_obj = model.loss
    loss_obj(y, pot)
    dpot_dev = loss_obj.backward()
    assert_close(host(dpot_dev), dpot, 1e-4, "dpot")
    model.backward(dpot_dev)
    got = {v.name: host(v.grad) for v in model.trainable_weights}
    assert_close(got[n[4]], dT, 2e-4, "transitions grad")
    if mode == "f32":
        d2 = dpot.reshape(-1, C)
        assert_close(got[n[2]], d2.T @ hdn, 2e-4, "dense2 grad")
        du = (d2 @ w[n[2]]) * ob.swish_grad(u)
        assert_close(got[n[0]], du.T @ x.reshape(-1, 768), 2e-4, "dense1 grad")
    else:
        for k in n[:4]:
            assert np.isfinite(got[k]).all() and np.abs(got[k]).max() > 0
    pot_inf = host(model(x, training=False))
    ref_tags = ol.crf_viterbi(host(pot).astype(np.float32), np.full(B, S), w[n[4]].astype(np.float32))
    assert pot_inf.shape == (B, S, C)
    assert np.array_equal(model.inference(x).cpu().numpy(), ref_tags)


def test_ner_crf_25_tags_sample_weights_and_mask():
    """CRF(C, mask_impossible_transitions=M) in a SequentialNERBertModel with loss_sample_weights."""
    from polus_amd.layers import CRF, Dense
    from polus_amd.ner.models import SequentialNERBertModel
    n_types = 12
    mask = bio_mask(n_types)
    C = mask.shape[0]                                            # 26
    B, S = 5, 20
    x, _ = _ner_inputs(11, B, S, C)
    r = rng(12)
    tags = r.integers(1, C, size=(B, S))
    tags[0] = 1                                                  # a sequence without positive classes
    y = np.eye(C, dtype=np.float32)[tags]
    crf = CRF(C, mask_impossible_transitions=mask)
    model = SequentialNERBertModel([Dense(C, input_shape=(S, 768), out_dtype=torch.float32), crf], compute_dtype="f32",
                                   input_dim=768)
    n = [v.name for v in model.trainable_weights]
    w = {v.name: v.numpy().astype(np.float64) for v in model.trainable_weights}
    mpc = np.ones(C, np.float32)
    mpc[:2] = 0                                                  # PAD and O are negatives
    lw = crf.loss_sample_weights(mpc, 0.25)
    pot = model(x, training=True)
    loss = float(lw(y, pot))
    sw = ol.crf_sample_weights(y, mpc, 0.25)
    assert sw[0] == 0.25 and (sw[1:] == 1).all()
    pot_ref = host(pot)
    loss_ref, dpot, dT = ol.crf_nll_fwd(y, pot_ref, np.full(B, S), w[n[2]], mask, sw)
    assert abs(loss - loss_ref) < 1e-4 * max(1.0, abs(loss_ref))
    dpot_dev = lw.backward()
    assert_close(host(dpot_dev), dpot, 1e-4, "weighted dpot")
    model.backward(dpot_dev)
    assert_close(host(model.trainable_weights[2].grad), dT, 2e-4, "masked transitions grad")
    masked = ol.crf_transitions(w[n[2]].astype(np.float32), mask)
    ref_tags = ol.crf_viterbi(pot_ref.astype(np.float32), np.full(B, S), masked)
    assert np.array_equal(model.inference(x).cpu().numpy(), ref_tags)


@pytest.mark.parametrize("dropout", [False, True])
def test_ner_crf_25_tags_trainer_steps(dropout):
    from polus_amd.ner.models import baselineNER_MLP_CRF, baselineNER_MLP_Dropout_CRF
    from polus_amd.optimizers import AdamWeightDecay
    from polus_amd.training import ClassifierTrainer
    B, S, C = 8, 32, 25
    x, y = _ner_inputs(21, B, S, C)
    if dropout:
        model = baselineNER_MLP_Dropout_CRF(sequence_length=S, output_classes=C, droupout_p=0.1, compute_dtype="bf16")
    else:
        model = baselineNER_MLP_CRF(sequence_length=S, output_classes=C)
    trainer = ClassifierTrainer(model, AdamWeightDecay(1e-3), model.loss)
    losses = [float(trainer.train_step(x, y)) for _ in range(3)]
    assert all(np.isfinite(losses)), losses
    if not dropout:
        assert losses[-1] < losses[0], losses
    out = model.inference(x).cpu().numpy()
    assert out.shape == (B, S) and out.min() >= 0 and out.max() < C
