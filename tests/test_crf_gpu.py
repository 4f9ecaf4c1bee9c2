"""GPU: both CRF kernel families behind ops.crf_nll / ops.crf_viterbi (loss.hip for C <= 16, crf.hip for 17 <= C <= 128)
against the float64 oracle on the case table of tests/crf_cases.py: both ends of each path and of each C_PAD bucket, a second
64-thread block, S beyond the workgroup, lengths and tags that clamp, lengths=None, garbage tags past L, sample weights with
an exact 0, accumulate, NaN-prefilled outputs and a 0xFF-filled workspace; S = 512 and confident emissions under a BIO mask
with bounds derived from the float32 restatements (tests/crf_ref.py); Viterbi exact on a dyadic grid with ties.  The
observed worst error of every case is printed beside its bound (pytest -s).

Before crf.hip recomputed underflowed sums in the log domain, the workgroup path floored them at FLT_MIN and the margin
cases from M = 95 on and the scale-100 cases failed here (12 of the 28; C = 16 runs on the log-domain kernels and passed).
The first assertion to fail was
    margin-C26-M95 loss: 1.2e-01 > 2.0e-05
and the worst figures were loss 2.3e+01 (margin-C26-M1000), dpot 1.56 and dtrans 0.78 of max|ref| (scale-C128-x100), each
equal to what the restatement of that arithmetic (crf_ref.nll_scaled) gives on the CPU.  With the rescues alone one case
still missed (scale-C64-x100 dpot 4.4e-03 > 4.0e-03: all-f32 rounding at |alpha| = 1.2e4); it passes since the scans keep
the shared part of alpha and beta in doubles (crf_ref.nll_split restates that)."""
import numpy as np
import pytest
import torch

from oracle import losses as ol
from tests import crf_cases as cc
from tests.util import dev, host

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def ops():
    from polus_amd import ops as _ops
    return _ops


def poison_workspace(ops, B, S, C):
    from polus_amd import _lib
    nb = _lib.load().polus_crf_workspace_bytes(B, S, C)
    ops.workspace(torch.device("cuda", torch.cuda.current_device())).get(nb).fill_(0xFF)


def run_nll(ops, inp, dtype="f32", weights=None, prior=None, lengths="own"):
    B, S, C = inp.shape
    loss = torch.full((1,), float("nan"), device="cuda")
    dpot = torch.full((B, S, C), float("nan"), device="cuda", dtype=DT[dtype])
    dT = dev(prior) if prior is not None else torch.full((C, C), float("nan"), device="cuda")
    pot, tags, trans = dev(inp.pot), dev(inp.tags), dev(inp.trans)
    L = None if lengths is None else dev(inp.lengths)
    w = None if weights is None else dev(weights)
    poison_workspace(ops, B, S, C)
    ops.crf_nll(pot, tags, L, trans, w, loss, dpot, dT, accumulate=prior is not None)
    return {"loss": float(loss), "dpot": host(dpot), "dtrans": host(dT)}


def check(name, got, ref, tol):
    """Print every figure, then assert."""
    for k in ("dpot", "dtrans"):
        assert np.isfinite(got[k]).all(), f"{name} {k}: not finite"
    assert np.isfinite(got["loss"]), f"{name} loss: not finite"
    err = cc.errors(got, ref)
    print(f"{name:34s} " + "  ".join(f"{k} {err[k]:.2e} / {tol[k]:.1e}" for k in err))
    for k in err:
        assert err[k] <= tol[k], f"{name} {k}: {err[k]:.1e} > {tol[k]:.1e}"
    return err


@pytest.mark.parametrize("B,S,C", cc.SHAPES, ids=lambda v: str(v))
def test_crf_nll_matches_oracle(ops, B, S, C):
    inp = cc.nll_inputs(B, S, C)
    Lc = inp.L
    for weights in (None, inp.weights):
        base = cc.reference(inp, weights)
        for prior in (None, inp.prior):
            ref = base if prior is None else {**base, "dtrans": base["dtrans"] + prior.astype(np.float64)}
            dT = {}
            for dtype in cc.DTYPES:
                name = f"{B}x{S}x{C} {dtype} w={weights is not None} acc={prior is not None}"
                got = run_nll(ops, inp, dtype, weights, prior)
                check(name, got, ref, cc.tolerances(dtype))
                for b in range(B):
                    assert not got["dpot"][b, Lc[b]:].any(), f"{name}: dpot[{b}, L:] is not zero"
                if weights is not None:
                    assert not got["dpot"][weights == 0].any(), f"{name}: a weight-0 sequence has a gradient"
                dT[dtype] = got["dtrans"]
            assert np.array_equal(dT["f32"], dT["bf16"]), "dtrans depends on the dpot dtype"
    ref = cc.reference(inp, inp.weights, lengths=None)
    for dtype in cc.DTYPES:
        check(f"{B}x{S}x{C} {dtype} lengths=None", run_nll(ops, inp, dtype, inp.weights, lengths=None), ref, cc.tolerances(dtype))


@pytest.mark.parametrize("B,S,C", cc.LONG_SHAPES, ids=lambda v: str(v))
def test_crf_nll_long_sequences(ops, B, S, C):
    inp = cc.long_inputs(B, S, C)
    got = run_nll(ops, inp)
    check(f"long {B}x{S}x{C}", got, cc.reference(inp), cc.LONG_TOL[(B, S, C)])
    assert not got["dpot"][1:, S - 37:].any()


@pytest.mark.parametrize("kind,n_types,v", cc.BIO_CASES, ids=lambda v: str(v))
def test_crf_nll_confident_emissions_under_bio_mask(ops, kind, n_types, v):
    """On the MI355X the workgroup path is within 0.32 of every margin bound (dpot <= 5.5e-5) and within 0.02 of every
    scale bound (scale 100: dpot <= 8.3e-5, dtrans <= 4.2e-5, where the log-domain kernels at C = 16 have 3.9e-3 and
    1.8e-3): crf.hip keeps the part of alpha and beta that all tags share in doubles, so its error does not grow with
    |alpha| as that of an all-f32 scan does."""
    inp = cc.bio_inputs(kind, n_types, v)
    got = run_nll(ops, inp)
    assert np.isfinite(got["dtrans"]).all(), "raw dtrans is not finite"
    name = f"{kind}-C{inp.shape[2]}-{'M' if kind == 'margin' else 'x'}{v}"
    again = run_nll(ops, inp)                                    # the rescues add in a fixed order too
    assert all(np.array_equal(got[k], again[k]) for k in got), "two runs differ"
    check(name, cc.bio_got(inp, got["loss"], got["dpot"], got["dtrans"]), cc.bio_reference(inp), cc.BIO_TOL[(kind, n_types, v)])


def run_viterbi(ops, pot, lengths, trans):
    B, S, C = pot.shape
    out = torch.full((B, S), -1, dtype=torch.int32, device="cuda")
    poison_workspace(ops, B, S, C)
    ops.crf_viterbi(dev(pot), None if lengths is None else dev(lengths), dev(trans), out)
    return out.cpu().numpy()


@pytest.mark.parametrize("B,S,C", cc.VITERBI_SHAPES, ids=lambda v: str(v))
def test_crf_viterbi_exact_with_ties(ops, B, S, C):
    pot, lengths, trans = cc.viterbi_inputs(B, S, C)
    Lc = cc.clamp_lengths(lengths, S)
    got = run_viterbi(ops, pot, lengths, trans)
    assert np.array_equal(got, ol.crf_viterbi(pot, Lc, trans))
    for b in range(B):
        assert not got[b, Lc[b]:].any()
    assert np.array_equal(run_viterbi(ops, pot, None, trans), ol.crf_viterbi(pot, np.full(B, S), trans))


@pytest.mark.parametrize("n_types", cc.BIO_TYPES)
def test_crf_viterbi_exact_under_bio_mask(ops, n_types):
    mask = cc.bio_mask(n_types)
    B, S, C = cc.VITERBI_BIO_B, cc.VITERBI_BIO_S, mask.shape[0]
    pot, lengths, trans = cc.viterbi_inputs(B, S, C, mask)
    Lc = cc.clamp_lengths(lengths, S)
    got = run_viterbi(ops, pot, lengths, trans)
    assert np.array_equal(got, ol.crf_viterbi(pot, Lc, trans))
    for b in range(B):
        assert all(mask[got[b, s - 1], got[b, s]] for s in range(1, Lc[b]))


def test_crf_arguments_of_another_type_or_layout_are_refused(ops):
    B, S, C = 2, 4, 5
    f = lambda *shape: torch.zeros(shape, device="cuda")
    i = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    good = dict(potentials=f(B, S, C), tags=i(B, S), lengths=i(B), trans=f(C, C), sample_w=f(B), loss=f(1),
                dpot=f(B, S, C), dtrans=f(C, C))
    ops.crf_nll(**good)
    bad = {"tags": [i(B, S).long(), i(S, B).t(), i(B, S + 1)], "lengths": [i(B).long(), i(2 * B)[::2], i(B + 1)],
           "trans": [f(C, C).t(), f(C, C).double(), f(C, C + 1)[:, :C]], "sample_w": [f(B).double(), f(2 * B)[::2]],
           "dtrans": [f(C, C).t(), f(C, C).bfloat16()], "loss": [f(1).double()], "potentials": [f(B, S, C).bfloat16()]}
    for k, vals in bad.items():
        for v in vals:
            with pytest.raises(AssertionError):
                ops.crf_nll(**{**good, k: v})
    vgood = dict(potentials=f(B, S, C), lengths=i(B), trans=f(C, C), out_tags=i(B, S))
    ops.crf_viterbi(**vgood)
    vbad = {"potentials": [f(B, S, C).bfloat16(), f(B, C, S).transpose(1, 2)], "lengths": [i(B).long()],
            "trans": [f(C, C).t(), f(C, C).double()], "out_tags": [i(B, S).long(), i(S, B).t()]}
    for k, vals in vbad.items():
        for v in vals:
            with pytest.raises(AssertionError):
                ops.crf_viterbi(**{**vgood, k: v})
    torch.cuda.synchronize()
