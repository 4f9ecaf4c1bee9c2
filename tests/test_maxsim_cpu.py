"""CPU: the float64 MaxSim reference (tests/maxsim_ref.py) against finite differences and its masking rules, the
MaxSim kernels (polus_amd/csrc/maxsim.hip) compile for gfx950 without scratch, the public names import, and every
GPU score tolerance of tests/maxsim_cases.py sits at least 5x below the score change of one wrong decision."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import maxsim_ref as ref
from tests.maxsim_cases import BENCH, MASKS, SHAPES, TOL, gap_floor, make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "polus_amd", "csrc", "maxsim.hip")


def test_reference_gradients_match_finite_differences():
    r = np.random.Generator(np.random.PCG64(2))
    B, N, Lq, Ld, E = 2, 3, 4, 6, 5
    q, d = r.standard_normal((B, Lq, E)), r.standard_normal((N, Ld, E))
    qm = np.ones((B, Lq), np.int32); qm[1, 3] = 0
    dm = np.ones((N, Ld), np.int32); dm[2, 4:] = 0
    w = r.standard_normal((B, N))
    f = lambda q_, d_: float((w * ref.maxsim_fwd(q_, d_, qm, dm)[0]).sum())
    _, am = ref.maxsim_fwd(q, d, qm, dm)
    assert ref.top2_gap(q, d, qm, dm)[am >= 0].min() > 1e-3          # away from ties: the argmax is locally fixed
    dq, dd = ref.maxsim_bwd(q, d, w, am)
    h = 1e-6
    for x, g in ((q, dq), (d, dd)):
        num = np.zeros_like(x)
        for idx in np.ndindex(x.shape):
            xp, xm = x.copy(), x.copy()
            xp[idx] += h; xm[idx] -= h
            args_p = (xp, d) if x is q else (q, xp)
            args_m = (xm, d) if x is q else (q, xm)
            num[idx] = (f(*args_p) - f(*args_m)) / (2 * h)
        assert np.abs(num - g).max() < 1e-6
    assert (dq[1, 3] == 0).all() and (dd[2, 4:] == 0).all()
    # normalisation: backward against finite differences of sum(v * y)
    x = r.standard_normal((3, 7))
    v = r.standard_normal((3, 7))
    gx = ref.l2norm_bwd(x, v)
    num = np.zeros_like(x)
    for idx in np.ndindex(x.shape):
        xp, xm = x.copy(), x.copy()
        xp[idx] += h; xm[idx] -= h
        num[idx] = ((v * ref.l2norm_fwd(xp)[0]).sum() - (v * ref.l2norm_fwd(xm)[0]).sum()) / (2 * h)
    assert np.abs(num - gx).max() < 1e-6
    y, rn = ref.l2norm_fwd(np.zeros((1, 4)))
    assert (y == 0).all() and rn[0] == 1e12
    assert np.allclose(ref.l2norm_bwd(np.zeros((1, 4)), np.ones((1, 4))), 1e12)


def test_reference_tie_empty_document_and_masked_query_rules():
    q = np.array([[[1.0, 0.0], [0.0, 1.0], [2.0, 2.0]]])           # B = 1, Lq = 3
    d = np.array([[[0.0, 1.0], [1.0, 0.0], [1.0, 0.0], [0.0, 1.0]],  # duplicates: ties go to the lowest j
                  [[5.0, 5.0], [1.0, 1.0], [0.0, 0.0], [0.0, 0.0]]])
    s, am = ref.maxsim_fwd(q, d)
    assert am[0, 0].tolist() == [1, 0, 0] and s[0, 0] == 1 + 1 + 2
    dm = np.array([[1, 1, 1, 1], [0, 0, 0, 0]])                      # document 1 has no valid token
    s, am = ref.maxsim_fwd(q, d, None, dm)
    assert (am[0, 1] == -1).all() and s[0, 1] == 0.0
    qm = np.array([[1, 0, 1]])                                       # query token 1 masked
    s, am = ref.maxsim_fwd(q, d, qm, None)
    assert am[0, 0].tolist() == [1, -1, 0] and s[0, 0] == 1 + 2 and s[0, 1] == 5 + 20
    qm0 = np.zeros((1, 3), np.int32)                                 # a query without a valid token
    s, am = ref.maxsim_fwd(q, d, qm0, None)
    assert (am == -1).all() and (s == 0).all()
    dq, dd = ref.maxsim_bwd(q, d, np.ones((1, 2)), am)
    assert (dq == 0).all() and (dd == 0).all()
    dm2 = np.array([[0, 1, 1, 1], [1, 1, 1, 1]])                     # a masked winner passes the win on
    s, am = ref.maxsim_fwd(q, d, None, dm2)
    assert am[0, 0].tolist() == [1, 3, 1]


@pytest.fixture(scope="module")
def maxsim_asm(tmp_path_factory):
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("maxsim") / "maxsim.s")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", SRC, "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return open(out).read()


def test_maxsim_kernels_have_no_scratch(maxsim_asm):
    segs = dict(re.findall(r"\.amdhsa_kernel\s+(\S+).*?\.amdhsa_private_segment_fixed_size\s+(\d+)", maxsim_asm, flags=re.S))
    names = set(segs)
    assert sum("maxsim_fwd_kernel" in n for n in names) == 16         # E / 32 in 1..8 x {f32, bf16}
    for k in ("maxsim_bwd_dq_kernel", "maxsim_bwd_dd_kernel", "l2norm_fwd_kernel", "l2norm_bwd_kernel"):
        assert sum(k in n for n in names) == 2, k
    for name, size in segs.items():
        assert int(size) == 0, f"{name}: private segment {size} B"
    bodies = {m.group(1): m.group(2) for m in
              re.finditer(r"^(_Z\w+):[^\n]*$(.*?)^\s*\.size\s+\1,", maxsim_asm, flags=re.M | re.S)}
    assert names <= set(bodies)
    for name in names:
        assert not re.search(r"^\s*scratch_", bodies[name], flags=re.M), f"{name} uses scratch_ instructions"


def test_public_names_import():
    from polus.ir.models import LateInteractionDualEncoder, TokenReps
    from polus.ir.training import EfficientDenseRetrievalTrainer, MaxSimScores
    assert issubclass(LateInteractionDualEncoder, object) and TokenReps._fields == ("values", "mask")
    assert MaxSimScores().normalize and callable(EfficientDenseRetrievalTrainer.forward_with_grads)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("masks", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_score_tolerance_sits_below_one_wrong_decision(shape, masks, mode):
    """On the data the GPU parity test uses (rounded as the device sees it), the smallest score change, among
    those above the argmax floor, of taking the second-best token / counting a masked token / dropping a query token
    is at least 5x the score tolerance."""
    import torch
    from tests.util import rounded
    q, d, qm, dm = make_case(shape, masks)
    dt = torch.float32 if mode == "f32" else torch.bfloat16
    qr, dr = rounded(q, dt), rounded(d, dt)
    sc = ref.error_scales(qr, dr, qm, dm, floor=gap_floor(qr, dr))
    for what, e in sc.items():
        assert TOL[mode]["score"] * 5 <= e, (what, e)


def test_score_tolerance_below_one_wrong_decision_bench_shape():
    import torch
    from tests.util import rounded
    for masks in ("none", "ragged"):
        q, d, qm, dm = make_case(BENCH, masks)
        qr, dr = rounded(q, torch.bfloat16), rounded(d, torch.bfloat16)
        sc = ref.error_scales(qr, dr, qm, dm, floor=gap_floor(qr, dr))
        for what, e in sc.items():
            assert TOL["bf16"]["score"] * 5 <= e, (what, e)
