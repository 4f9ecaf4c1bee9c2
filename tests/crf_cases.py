"""Cases for the linear-chain CRF (polus_amd/csrc/loss.hip crf_nll_kernel / crf_viterbi_kernel, one thread per sequence,
C <= 16; polus_amd/csrc/crf.hip crf_nll_wg_kernel / crf_viterbi_wg_kernel, one workgroup per sequence, 17 <= C <= 128 in
buckets C_PAD of 32, 64, 128), shared by the oracle test of both paths (test_crf_gpu.py) and by the CPU check that the
tolerances can see an off-by-one length, transposed transitions or a floored underflow (test_crf_cases_cpu.py).  No GPU
needed to import.

The reference of every assertion on device output is oracle/losses.py in float64 (crf_nll_fwd, crf_viterbi,
crf_transitions) on the inputs the device sees, with lengths and tags clamped as the kernels clamp them.

Tolerances.  LOSS_TOL, DPOT_TOL, DTRANS_TOL are the suite's bounds (test_kernels_gpu.py, test_crf_large_gpu.py).  The
long sequences and the confident-emission cases cannot be held to them in f32 whatever the formulation; their bounds are
derived from the float32 restatements of tests/crf_ref.py against the oracle (derived_tol below), never from a kernel,
and the measured restatement errors are tabulated beside them (LONG_MEASURED, BIO_MEASURED)."""
from dataclasses import dataclass

import numpy as np

from oracle import losses as ol

CRF_MAXC = 16                       # loss.hip: one thread per sequence up to here
SMALL_SHAPES = ((1, 1, 1), (3, 7, 2), (4, 33, 9), (65, 9, 5), (130, 5, 16))
WG_SHAPES = ((3, 7, 17), (5, 9, 32), (4, 6, 33), (3, 5, 64), (2, 5, 65), (2, 4, 128), (3, 130, 20), (2, 131, 128))
SHAPES = SMALL_SHAPES + WG_SHAPES
DTYPES = ("f32", "bf16")
LENGTH_CLASSES = ("S", "0", "1", "2", "S-1", "S+5", "-3")
PAST_L_TAG = 2 ** 30                # every tag position at or past L

LOSS_TOL = 2e-5                     # of max(1, |ref|)
DPOT_TOL = {"f32": 1e-4, "bf16": 5e-3}      # of max|ref|; bf16: the f32 gradient rounded once, 2^-9 relative
DTRANS_TOL = 2e-4                   # of max|ref|
FLOOR = {"loss": LOSS_TOL, "dpot": DPOT_TOL["f32"], "dtrans": DTRANS_TOL}


def bucket(C):
    """C_PAD of crf.hip (crf_bucket); 0 on the one-thread-per-sequence path."""
    return 0 if C <= CRF_MAXC else (32 if C <= 32 else (64 if C <= 64 else 128))


def workgroup(C):
    """Threads per workgroup of crf_nll_wg_kernel (CrfCfg::NT)."""
    return max(64, bucket(C))


def rng(*key):
    return np.random.Generator(np.random.PCG64(list(key)))


# ------------------------------------------------------------------------------------------------- inputs
def phase(B, S, C):
    """Where a shape's lengths start in the cycle of classes: its place in the table, so that the small batches of the
    workgroup path reach every class between them."""
    return SHAPES.index((B, S, C)) if (B, S, C) in SHAPES else 0


def raw_lengths(B, S, seed=0, phase=0):
    """int32 [B] as passed to the device: S, then the other classes of LENGTH_CLASSES in turn from `phase` on, then
    random ones in [0, S]."""
    cyc = (0, 1, 2, S - 1, S + 5, -3)
    r = rng(B, S, seed, 1)
    return np.array([S if b == 0 else cyc[(b - 1 + phase) % 6] if b < 7 else r.integers(0, S + 1) for b in range(B)], np.int32)


def length_classes(B, phase=0):
    return {"S"} | {LENGTH_CLASSES[1 + (b - 1 + phase) % 6] for b in range(1, min(B, 7))}


def clamp_lengths(L, S):
    return np.clip(L, 0, S).astype(np.int32)


def raw_tags(B, S, C, Lc, seed=0):
    """int32 [B, S] as passed to the device and the positions [(b, s, value)] that are out of range inside L: in range
    inside the clamped length Lc, but for one -1 and one C + 3 per batch; PAST_L_TAG at and past L."""
    r = rng(B, S, C, seed, 2)
    t = r.integers(0, C, size=(B, S)).astype(np.int32)
    spots = [(b, s) for b in range(B) for s in sorted({0, int(Lc[b]) - 1}) if Lc[b] > 0]
    oor = []
    if spots:
        oor.append(spots[-1] + (-1,))
        if len(spots) > 1:
            oor.append(spots[0] + (C + 3,))
    for b, s, v in oor:
        t[b, s] = v
    for b in range(B):
        t[b, int(Lc[b]):] = PAST_L_TAG
    return t, oor


def clamp_tags(t, C):
    return np.clip(t, 0, C - 1).astype(np.int32)


def sample_weights(Lc, seed=0):
    """f32 [B] in [0.5, 1.5) with one exact 0: on the last non-empty sequence, or on the only one."""
    B = len(Lc)
    w = rng(B, seed, 3).uniform(0.5, 1.5, size=B).astype(np.float32)
    w[max(b for b in range(B) if Lc[b] > 0 or b == 0)] = 0.0
    return w


@dataclass
class Inputs:
    pot: np.ndarray                 # f32 [B, S, C]
    tags: np.ndarray                # int32 [B, S], raw
    lengths: np.ndarray             # int32 [B], raw
    trans: np.ndarray               # f32 [C, C], masked already where a mask applies
    weights: np.ndarray             # f32 [B]
    prior: np.ndarray               # f32 [C, C]: dtrans before an accumulate call
    oor: list
    mask: np.ndarray = None         # BIO cases: [C, C] of 0 / 1

    @property
    def shape(self):
        return self.pot.shape

    @property
    def L(self):
        return clamp_lengths(self.lengths, self.pot.shape[1])

    @property
    def t(self):
        return clamp_tags(self.tags, self.pot.shape[2])


def nll_inputs(B, S, C):
    """Potentials N(-d, 2^2), transitions N(0, 0.5^2).  d = log C + 4.25 / 2 is about what one step adds to alpha at d = 0
    (log of C terms exp(N(0, 4.25))), so that alpha, beta and logZ stay within tens at any S of the table: the marginals
    are exp(alpha + beta - logZ), an f32 alpha near 800 (S = 130 without the shift) is known to 6e-5 alone, and the 1e-4
    bound would then measure the format, as it does in the long cases, which derive their bounds for that reason.  The
    shift changes no gradient.  test_crf_cases_cpu.py holds both float32 restatements to half of every bound here."""
    r = rng(B, S, C, 4)
    lengths = raw_lengths(B, S, phase=phase(B, S, C))
    tags, oor = raw_tags(B, S, C, clamp_lengths(lengths, S))
    pot = r.standard_normal((B, S, C)) * 2 - (np.log(C) + 2.125)
    return Inputs(pot=pot.astype(np.float32), tags=tags, lengths=lengths,
                  trans=(r.standard_normal((C, C)) * 0.5).astype(np.float32), weights=sample_weights(clamp_lengths(lengths, S)),
                  prior=r.standard_normal((C, C)).astype(np.float32), oor=oor)


def reference(inp, weights=None, prior=None, lengths="own", mask=None):
    """oracle.losses.crf_nll_fwd in float64 on clamped tags and lengths: loss, dpot, dtrans (+ prior).  lengths=None:
    every sequence has length S, and the tags past the raw length clamp to C - 1."""
    B, S, C = inp.shape
    L = np.full(B, S, np.int32) if lengths is None else inp.L
    T = inp.trans.astype(np.float64)
    if mask is not None:
        T = np.where(mask != 0, T, 0.0)         # crf_nll_fwd masks once more: the same matrix
    loss, dx, dT = ol.crf_nll_fwd(np.eye(C)[inp.t], inp.pot.astype(np.float64), L, T, mask,
                                  None if weights is None else weights.astype(np.float64))
    if prior is not None:
        dT = dT + prior.astype(np.float64)
    return {"loss": float(loss), "dpot": dx, "dtrans": dT}


def errors(got, ref):
    """{output: error in the unit its tolerance is stated in}."""
    rel = lambda a, r: float(np.abs(np.asarray(a, np.float64) - r).max() / (np.abs(r).max() + 1e-30))
    return {"loss": abs(float(got["loss"]) - ref["loss"]) / max(1.0, abs(ref["loss"])),
            "dpot": rel(got["dpot"], ref["dpot"]), "dtrans": rel(got["dtrans"], ref["dtrans"])}


def tolerances(dtype="f32"):
    return {"loss": LOSS_TOL, "dpot": DPOT_TOL[dtype], "dtrans": DTRANS_TOL}


def derived_tol(*measured):
    """Twice the largest restatement error (the factor covers another summation order), floored at the suite's bound."""
    return {k: max(FLOOR[k], 2.0 * max(m[k] for m in measured)) for k in FLOOR}


# ------------------------------------------------------------------------------------------------- long sequences
LONG_SHAPES = ((2, 512, 5), (2, 512, 16), (2, 512, 17), (1, 512, 128))
# errors of crf_ref.nll_log / crf_ref.nll_scaled against the oracle on long_inputs (loss: of max(1, |ref|); dpot,
# dtrans: of max|ref|), rounded up to two digits; test_crf_cases_cpu.py re-measures them
LONG_MEASURED = {
    (2, 512, 5): {"log": {"loss": 9.8e-07, "dpot": 0.0012, "dtrans": 0.0014},
                  "scaled": {"loss": 3.7e-07, "dpot": 0.0028, "dtrans": 0.00021}},
    (2, 512, 16): {"log": {"loss": 1.5e-07, "dpot": 0.00099, "dtrans": 0.0002},
                  "scaled": {"loss": 6.6e-08, "dpot": 0.0019, "dtrans": 0.0007}},
    (2, 512, 17): {"log": {"loss": 2.2e-07, "dpot": 0.0013, "dtrans": 0.00046},
                  "scaled": {"loss": 2.2e-07, "dpot": 0.0016, "dtrans": 0.00022}},
    (1, 512, 128): {"log": {"loss": 8.3e-08, "dpot": 0.00056, "dtrans": 0.00013},
                  "scaled": {"loss": 2.3e-07, "dpot": 0.0016, "dtrans": 0.00045}},
}
LONG_TOL = {shape: derived_tol(*m.values()) for shape, m in LONG_MEASURED.items()}


def long_inputs(B, S, C):
    r = rng(B, S, C, 5)
    lengths = np.array([S, S - 37][:B], np.int32)
    tags, _ = raw_tags(B, S, C, lengths, seed=5)
    return Inputs(pot=(r.standard_normal((B, S, C)) * 2).astype(np.float32), tags=clamp_tags(tags, C), lengths=lengths,
                  trans=(r.standard_normal((C, C)) * 0.5).astype(np.float32), weights=None, prior=None, oor=[])


# ------------------------------------------------------------------------------------------------- BIO mask
BIO_TYPES = (7, 12, 31, 63)         # C = 16 (one thread per sequence), 26, 64, 128
MARGINS = (20, 60, 95, 200, 1000)
SCALES = (30, 100)
MARGIN_S, SCALE_S, BIO_B = 12, 48, 2
PAD, O, B0, I0 = 0, 1, 2, 3


def bio_mask(n_types):
    """PAD, O, then B-X / I-X for each type: I-X may only follow B-X or I-X."""
    C = 2 + 2 * n_types
    m = np.ones((C, C), np.float32)
    for i in range(n_types):
        ix = 3 + 2 * i
        m[:, ix] = 0
        m[ix - 1, ix] = m[ix, ix] = 1
    return m


def obey(tags):
    """An I-X that follows neither B-X nor I-X becomes B-X."""
    tags = tags.copy()
    for b in range(tags.shape[0]):
        for s in range(tags.shape[1]):
            t = tags[b, s]
            if t >= 3 and t % 2 == 1 and (s == 0 or tags[b, s - 1] not in (t - 1, t)):
                tags[b, s] = t - 1
    return tags


def _bio(n_types, key, S):
    mask = bio_mask(n_types)
    C = mask.shape[0]
    r = rng(n_types, key, S, 6)
    trans = ol.crf_transitions((r.standard_normal((C, C)) * 0.5).astype(np.float32), mask)
    return mask, C, r, trans


def margin_inputs(n_types, M):
    """Standard-normal emissions, +M on O at step 4 and +M on I-0 at step 5; gold O ... B-0 I-0 ... O.  Every path
    through (O, I-0) is masked, so the partition function is carried by tags far below step 4's best one."""
    mask, C, r, trans = _bio(n_types, M, MARGIN_S)
    pot = r.standard_normal((BIO_B, MARGIN_S, C)).astype(np.float32)
    pot[:, 4, O] += M
    pot[:, 5, I0] += M
    tags = np.full((BIO_B, MARGIN_S), O, np.int32)
    tags[:, 4], tags[:, 5] = B0, I0
    return Inputs(pot=pot, tags=tags, lengths=np.full(BIO_B, MARGIN_S, np.int32), trans=trans, weights=None, prior=None,
                  oor=[], mask=mask)


def scale_inputs(n_types, scale):
    mask, C, r, trans = _bio(n_types, scale, SCALE_S)
    pot = (r.standard_normal((BIO_B, SCALE_S, C)) * scale).astype(np.float32)
    tags = obey(r.integers(1, C, size=(BIO_B, SCALE_S)).astype(np.int32))
    return Inputs(pot=pot, tags=tags, lengths=np.array([SCALE_S, SCALE_S - 5], np.int32), trans=trans, weights=None,
                  prior=None, oor=[], mask=mask)


BIO_CASES = [("margin", n, M) for n in BIO_TYPES for M in MARGINS] + [("scale", n, sc) for n in BIO_TYPES for sc in SCALES]


def bio_inputs(kind, n_types, v):
    return margin_inputs(n_types, v) if kind == "margin" else scale_inputs(n_types, v)


def bio_reference(inp):
    return reference(inp, mask=inp.mask)


def bio_got(inp, loss, dpot, dtrans):
    """dtrans * mask, as the layer applies it."""
    return {"loss": loss, "dpot": dpot, "dtrans": np.asarray(dtrans, np.float64) * inp.mask}


# errors of crf_ref.nll_log (the log-domain arithmetic: the correct one here) against the oracle on bio_inputs, rounded up
# to two digits: (loss, dpot, dtrans)
BIO_MEASURED = {
    ("margin", 7, 20): (4.1e-09, 5.4e-06, 3.1e-07),
    ("margin", 7, 60): (4.7e-07, 9.7e-06, 4.3e-07),
    ("margin", 7, 95): (2.3e-07, 3.2e-06, 3.8e-07),
    ("margin", 7, 200): (3e-08, 7e-06, 4.8e-07),
    ("margin", 7, 1000): (3.1e-06, 8.8e-05, 2.1e-06),
    ("margin", 12, 20): (1.2e-07, 3.1e-06, 6e-08),
    ("margin", 12, 60): (1.2e-07, 4.3e-06, 1.8e-07),
    ("margin", 12, 95): (1.4e-07, 1.5e-05, 4.4e-07),
    ("margin", 12, 200): (1.2e-06, 9.3e-06, 3.8e-07),
    ("margin", 12, 1000): (1.6e-06, 8.7e-05, 1.3e-06),
    ("margin", 31, 20): (5.4e-08, 7.3e-06, 4.6e-08),
    ("margin", 31, 60): (1.5e-07, 8.1e-06, 7e-08),
    ("margin", 31, 95): (2.2e-07, 5.4e-06, 1.8e-07),
    ("margin", 31, 200): (5.2e-07, 6.2e-06, 1.6e-07),
    ("margin", 31, 1000): (8.6e-07, 0.00013, 6.9e-07),
    ("margin", 63, 20): (4.5e-08, 8.2e-06, 8.4e-08),
    ("margin", 63, 60): (6e-08, 8.4e-06, 1.2e-07),
    ("margin", 63, 95): (3.2e-08, 2.6e-06, 8.2e-08),
    ("margin", 63, 200): (8.9e-08, 1.1e-05, 1.1e-07),
    ("margin", 63, 1000): (2.6e-06, 7e-05, 1.1e-06),
    ("scale", 7, 30): (1.1e-07, 0.00052, 0.00015),
    ("scale", 7, 100): (2.4e-07, 0.0039, 0.0018),
    ("scale", 12, 30): (2.6e-07, 0.00077, 0.00062),
    ("scale", 12, 100): (6.3e-08, 0.0033, 0.0012),
    ("scale", 31, 30): (1.1e-07, 0.00092, 0.00046),
    ("scale", 31, 100): (9.8e-08, 0.002, 0.00098),
    ("scale", 63, 30): (2.5e-08, 0.00098, 0.00049),
    ("scale", 63, 100): (8.9e-09, 0.0049, 0.0025),
}
BIO_TOL = {case: derived_tol(dict(zip(("loss", "dpot", "dtrans"), m))) for case, m in BIO_MEASURED.items()}


# ------------------------------------------------------------------------------------------------- Viterbi
VITERBI_SHAPES = tuple(s for s in SHAPES if s[2] >= 4)
VITERBI_BIO_B, VITERBI_BIO_S = 3, 48


def viterbi_inputs(B, S, C, mask=None):
    """A dyadic grid (potentials k / 16 in [-4, 4], transitions k / 16 in [-0.5, 0.5]): every path sum is exact in f32 and
    in float64, so ties fall by the tie-break alone; the last three tags duplicate the first three."""
    r = rng(B, S, C, 7)
    pot = (r.integers(-64, 65, size=(B, S, C)) / 16.0).astype(np.float32)
    trans = (r.integers(-8, 9, size=(C, C)) / 16.0).astype(np.float32)
    pot[:, :, C - 3:] = pot[:, :, :3].copy()
    trans[C - 3:, :] = trans[:3, :].copy()
    trans[:, C - 3:] = trans[:, :3].copy()
    if mask is not None:
        trans = ol.crf_transitions(trans, mask)
    return pot, raw_lengths(B, S, seed=7, phase=phase(B, S, C)), trans
