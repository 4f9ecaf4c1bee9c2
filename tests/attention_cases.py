"""Attention cases shared by the oracle test of every kernel path (test_attention_gpu.py) and by the CPU check that its
tolerances can see an off-by-one key or dropout index (test_attention_cases_cpu.py).  No GPU needed to import.

Kernel paths (polus_amd/csrc/attention.hip polus_attention_fwd / polus_attention_bwd):
  F1  attn_fwd_dma_kernel<4>            bf16, S < 96
  F2  attn_fwd_dma_kernel<8>            bf16, 96 <= S <= 1024
  F3  attn_fwd_kernel<bf16, 8>          bf16, S > 1024
  F4  attn_fwd_kernel<float, 4>         f32
  B1  attn_bwd_fused_kernel<4>          bf16, S = 64
  B2  attn_bwd_fused_kernel<8>          bf16, S = 128
  B3  attn_bwd_q64_kernel<16>           bf16, S = 256
  B4  attn_bwd_kres_kernel, one block   bf16, S = 256 with POLUS_ATTN_BWD_KRES=2
  B5  attn_bwd_kres_kernel + dQ slabs   bf16, S % 256 == 0, 512 <= S <= 2048
  B6  attn_bwd_dq_kernel + _dkv_kernel  bf16, every other S, or POLUS_ATTN_FUSED=0
  B7  the same, f32                     f32

A case is one batch: every sample carries its own key mask (prefix lengths 1 and 2, lengths one below / at / one above
16, 32, 64, 128 and 256, left padding, holes with the last key kept, an all-zero mask, a full mask), or the whole batch
runs with mask=None.  The query rows are never masked (BERT), and dctx is non-zero on every row, padded ones included.
Each sample's edge keys (its last kept key and the padded key next to the kept region) score above the other keys
and carry large, distinct V rows, so that one key too many or too few moves the outputs far past the tolerances
(checked on the CPU)."""
import math
from dataclasses import dataclass, field

import numpy as np

from oracle import bert as ob
from tests.util import dropout_keep_np, elem_err, relerr

PATHS = {
    "F1": "attn_fwd_dma_kernel<4> (bf16, S < 96)",
    "F2": "attn_fwd_dma_kernel<8> (bf16, 96 <= S <= 1024)",
    "F3": "attn_fwd_kernel<bf16, 8> (bf16, S > 1024)",
    "F4": "attn_fwd_kernel<float, 4> (f32)",
    "B1": "attn_bwd_fused_kernel<4> (bf16, S = 64)",
    "B2": "attn_bwd_fused_kernel<8> (bf16, S = 128)",
    "B3": "attn_bwd_q64_kernel<16> (bf16, S = 256)",
    "B4": "attn_bwd_kres_kernel, one key block (bf16, S = 256, POLUS_ATTN_BWD_KRES=2)",
    "B5": "attn_bwd_kres_kernel + attn_bwd_dq_finish_kernel (bf16, S = 512..2048, S % 256 == 0)",
    "B6": "attn_bwd_dq_kernel + attn_bwd_dkv_kernel (bf16)",
    "B7": "attn_bwd_dq_kernel + attn_bwd_dkv_kernel (f32)",
}


def fwd_path(dtype, S):
    if dtype == "f32":
        return "F4"
    return "F1" if S < 96 else ("F2" if S <= 1024 else "F3")


def bwd_path(dtype, S, fused=1, kres=1):
    """The host-side selection of polus_attention_bwd, restated."""
    if dtype == "f32":
        return "B7"
    if fused and kres and S % 256 == 0 and S <= 2048 and (S > 256 or kres >= 2):
        return "B5" if S > 256 else "B4"
    if fused and S == 256:
        return "B3"
    if fused and S in (64, 128):
        return "B1" if S == 64 else "B2"
    return "B6"


# Tolerances per path and output: (max-relative, per-element).  The max-relative bound is |a - r|max <= tol * max|r|
# (tests/util.py assert_close); the per-element bound is |a - r| <= t * |r| + t * rms(r) for every element
# (assert_close_elem with rtol = atol_rms = t).  lse: absolute (1.1e-3 measured: the all-zero-mask rows sit at -10000,
# where f32 spacing is ~1e-3).  Each is 2-3x the worst error measured on MI355X over the cases below (bf16: rounding of
# the stored ctx / dQKV and of P' and dS to bf16 before their MFMAs, larger per element where long rows make small
# gradients; f32: the -10000 scores of the all-zero-mask samples); test_attention_cases_cpu.py holds each one to a 5x
# margin under the smallest error it must catch.
_BF16_LSE = 3e-3
TOL = {
    "F1": {"ctx": (1.2e-2, 1.2e-2), "lse": _BF16_LSE},
    "F2": {"ctx": (1.2e-2, 1.5e-2), "lse": _BF16_LSE},
    "F3": {"ctx": (1e-2, 1.2e-2), "lse": _BF16_LSE},
    "F4": {"ctx": (2e-4, 4e-4), "lse": 3e-3},
    "B1": {"dq": (1.2e-2, 3e-2), "dk": (1e-2, 7e-2), "dv": (1e-2, 6e-2)},
    "B2": {"dq": (1.2e-2, 5e-2), "dk": (1e-2, 0.15), "dv": (1e-2, 0.1)},
    "B3": {"dq": (1.3e-2, 9e-2), "dk": (1e-2, 0.2), "dv": (1e-2, 0.15)},
    "B4": {"dq": (1.3e-2, 0.11), "dk": (1e-2, 0.16), "dv": (1e-2, 0.15)},
    "B5": {"dq": (1.3e-2, 5e-2), "dk": (1e-2, 0.37), "dv": (1e-2, 0.25)},
    "B6": {"dq": (1.6e-2, 5e-2), "dk": (1.4e-2, 0.13), "dv": (1.2e-2, 0.13)},
    "B7": {"dq": (7e-4, 1.6e-3), "dk": (5e-4, 3e-3), "dv": (1.5e-4, 2e-3)},
}


@dataclass
class Case:
    dtype: str                    # "bf16" | "f32"
    S: int
    A: int
    masks: tuple                  # one spec per sample (see mask_row), or ("none",) * B for mask=None
    p: float = 0.0
    env: tuple = ()               # (("POLUS_ATTN_FUSED", 0), ...)
    seed: int = 0
    fwd: str = field(init=False)
    bwd: str = field(init=False)

    def __post_init__(self):
        e = dict(self.env)
        self.fwd = fwd_path(self.dtype, self.S)
        self.bwd = bwd_path(self.dtype, self.S, int(e.get("POLUS_ATTN_FUSED", 1)), int(e.get("POLUS_ATTN_BWD_KRES", 1)))

    @property
    def B(self):
        return len(self.masks)

    @property
    def no_mask(self):
        return self.masks[0] == "none"

    @property
    def name(self):
        env = "".join(f"-{k.split('_')[-1].lower()}{v}" for k, v in self.env)
        kind = "nomask" if self.no_mask else "+".join(self.masks) if len(self.masks) <= 3 else f"{self.B}masks"
        return f"{self.fwd}{self.bwd}-{self.dtype}-S{self.S}-A{self.A}-p{self.p}{env}-{kind}"


def mask_row(spec, S, rng):
    """One sample's key mask: 'len:L' (keys < L), 'left:P' (P leading zeros), 'holes' (interior zeros, the last key
    kept), 'zero', 'full'."""
    m = np.ones(S, np.int32)
    kind, _, arg = spec.partition(":")
    if kind == "len":
        m[int(arg):] = 0
    elif kind == "left":
        m[:int(arg)] = 0
    elif kind == "holes":
        m[rng.random(S) < 0.3] = 0
        m[min(15, S - 3):min(18, S - 1)] = 0       # a run of zeros across the 16-key edge
        m[S // 2] = 0
        m[-1] = 1
        m[0] = 1
    elif kind == "zero":
        m[:] = 0
    else:
        assert kind in ("full", "none"), spec
    return m


def edge_keys(m):
    """(last kept key, padded key next to the kept region) of one mask row; None where there is none."""
    kept = np.nonzero(m)[0]
    pad = np.nonzero(m == 0)[0]
    last = int(kept[-1]) if kept.size else None
    if not pad.size:
        first_pad = None
    elif kept.size and m[0] == 0 and kept[0] > 0 and not (m[kept[0]:] == 0).any():
        first_pad = int(kept[0]) - 1                # left padding: the zero just before the kept keys
    else:
        first_pad = int(pad[0])
    return last, first_pad


def mask_set(S):
    """Every mask kind that fits in rows of S keys."""
    specs = ["len:1", "len:2"]
    for e in (16, 32, 64, 128, 256):
        specs += [f"len:{L}" for L in (e - 1, e, e + 1) if L < S and f"len:{L}" not in specs]
    return specs + [f"left:{S // 3 + 1}", "holes", "zero", "full"]


def _chunks(specs, S, A, limit=16 << 20):
    per = max(1, limit // (A * S * S))
    return [tuple(specs[i:i + per]) for i in range(0, len(specs), per)]


def _cases():
    out = []

    def add(dtype, S, A, p, specs, env=(), nomask_B=0):
        for ch in _chunks(specs, S, A):
            out.append(Case(dtype, S, A, ch, p, env, seed=len(out) * 7919 + S))
        if nomask_B:
            out.append(Case(dtype, S, A, ("none",) * nomask_B, p, env, seed=len(out) * 7919 + S))

    # short rows: every mask kind, every dropout setting
    for dtype, S, A, env in (("f32", 17, 2, ()), ("f32", 50, 1, ()), ("f32", 128, 1, ()),
                             ("bf16", 17, 2, ()), ("bf16", 50, 2, ()), ("bf16", 64, 2, ()), ("bf16", 128, 2, ()),
                             ("bf16", 200, 1, ()), ("bf16", 256, 12, ()), ("bf16", 256, 12, (("POLUS_ATTN_BWD_KRES", 2),)),
                             ("bf16", 128, 2, (("POLUS_ATTN_FUSED", 0),))):
        for p in (0.0, 0.1, 0.5):
            add(dtype, S, A, p, mask_set(S), env, nomask_B=2 if dtype == "bf16" and p != 0.5 else 0)
    # long rows (B5 with 3, 4 and 8 slabs, F3 and B6 at 1088): every mask kind once, a few with dropout
    add("bf16", 768, 1, 0.0, mask_set(768), nomask_B=1)
    add("bf16", 768, 1, 0.1, ["len:1", "len:257", "holes", "left:300"])
    add("bf16", 768, 1, 0.5, ["len:2", "len:255", "zero", "full"])
    add("bf16", 1088, 1, 0.0, mask_set(1088), nomask_B=1)
    add("bf16", 1088, 1, 0.1, ["len:1", "len:129", "holes", "left:500"])
    add("bf16", 1088, 1, 0.5, ["len:2", "len:256", "zero", "full"])
    add("bf16", 1024, 1, 0.1, ["len:1", "len:1023", "holes", "left:257"], nomask_B=1)
    add("bf16", 1024, 1, 0.5, ["len:33", "zero", "full"])
    add("bf16", 2048, 1, 0.0, ["len:2", "len:1025", "holes"], nomask_B=1)
    add("bf16", 2048, 1, 0.1, ["len:1", "left:1500", "full"])
    add("bf16", 2048, 1, 0.5, ["len:257", "zero", "holes"])
    return out


CASES = _cases()


def make_inputs(case):
    """qkv [B, S, 3H], mask [B, S] int32 (all ones for mask=None), dctx [B, S, H] (float64, not yet rounded)."""
    r = np.random.Generator(np.random.PCG64(case.seed))
    B, S, H = case.B, case.S, case.A * 64
    qkv = r.standard_normal((B, S, 3 * H)) * 0.7
    dctx = r.standard_normal((B, S, H))
    mask = np.stack([mask_row(s, S, r) for s in case.masks])
    u = r.standard_normal((case.A, 64))
    u = (u / np.linalg.norm(u, axis=1, keepdims=True)).reshape(H)
    qkv[..., :H] += 4.0 * u                           # every query leans along u (per head) ...
    for b in range(B):
        boost = max(0.0, math.log(max(int(mask[b].sum()), 1)) - 1.0)
        for j, key in enumerate(edge_keys(mask[b])):
            if key is not None:                       # ... the edge keys' scores sit ~boost above the others (they
                qkv[b, key, H:2 * H] += 2.0 * boost * u   # carry ~1/4 of a long row), their V rows large and distinct
                qkv[b, key, 2 * H:] = (3.0 + j) * np.where(r.random(H) < 0.5, -1.0, 1.0)
    return qkv, mask, dctx


def keep_scale(case, idx0=0, key_major=False):
    """Oracle dropout scale [B, A, S, S]: element (b, h, q, key) is kept by the hash of ((b A + h) S + q) S + key."""
    B, A, S = case.B, case.A, case.S
    k = dropout_keep_np(case.seed, case.p, idx0, B * A * S * S).reshape(B, A, S, S).astype(np.float64) / (1.0 - case.p)
    return np.ascontiguousarray(k.transpose(0, 1, 3, 2)) if key_major else k


def oracle(qkv_r, mask, dctx_r, A, keep=None, ctx_in=None):
    """float64 ctx [B, S, H], lse [B, A, S] (natural log of the masked scaled scores) and dqkv [B, S, 3H].

    ctx_in: the ctx the backward is given (an input of polus_attention_bwd, stored in the engine's dtype).  The backward
    takes delta_q = sum_d dctx[q, d] ctx_in[q, d], where oracle/bert.py attention_bwd sums dP'*P exactly; the difference
    moves dS = P (dP' - delta) by P * (delta_exact - delta_in) / 8, which is added here.  It matters where one key holds
    a row (P = 1, exact dS = 0) under a dropout scale that bf16 cannot hold (1 / 0.9): there it is all of dS."""
    B, S, H3 = qkv_r.shape
    H = H3 // 3
    add = ob.additive_mask(mask, np.float64)
    ctx, probs = ob.attention_fwd(qkv_r, add, A, keep)
    q = qkv_r[..., :H].reshape(B, S, A, 64).transpose(0, 2, 1, 3)
    k = qkv_r[..., H:2 * H].reshape(B, S, A, 64).transpose(0, 2, 1, 3)
    sc = q @ k.transpose(0, 1, 3, 2) / math.sqrt(64) + add
    mx = sc.max(-1, keepdims=True)
    lse = (mx + np.log(np.exp(sc - mx).sum(-1, keepdims=True)))[..., 0]
    dqkv = ob.attention_bwd(dctx_r, qkv_r, probs, A, keep)
    if ctx_in is not None:
        heads = lambda x: x.reshape(B, S, A, 64).transpose(0, 2, 1, 3)
        dd = (heads(dctx_r) * heads(ctx - np.asarray(ctx_in, np.float64).reshape(ctx.shape))).sum(-1)   # [B, A, S]
        ds = probs * dd[..., None] / math.sqrt(64)
        dqkv[..., :H] += (ds @ k).transpose(0, 2, 1, 3).reshape(B, S, H)
        dqkv[..., H:2 * H] += (ds.transpose(0, 1, 3, 2) @ q).transpose(0, 2, 1, 3).reshape(B, S, H)
    return ctx, lse, dqkv


def split(dqkv, H):
    return {"dq": dqkv[..., :H], "dk": dqkv[..., H:2 * H], "dv": dqkv[..., 2 * H:]}


def violation(actual, ref, tol):
    """How far past the bounds of `tol` = (max-relative, per-element) `actual` lies: the larger of the two ratios
    (<= 1 passes both checks)."""
    mr, t = tol
    return max(relerr(actual, ref) / mr, elem_err(actual, ref, t, t))
