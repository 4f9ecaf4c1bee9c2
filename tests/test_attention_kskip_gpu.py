"""Key-block skipping (POLUS_ATTN_KSKIP) of attn_fwd_dma_kernel<4 / 8>, attn_bwd_fused_kernel<4 / 8> and
attn_bwd_q64_kernel<16>: switch on against switch off in one process, ctx, lse and dqkv compared as raw bits.

With the switch on a (batch, head) stops at the key block that holds its last unmasked key.  That keeps every bit because
a padded key scores s * scale - 10000 and its probability is exp(that - row max): an exact +0 in f32 once the row has one
unmasked key and |scaled scores| stay far below 10 000.  The inputs are built the way tests/attention_cases.py builds its
own (make_inputs: N(0, 0.7) entries, queries leaning along one direction, edge keys boosted by at most
2 (ln S - 1) <= 9.1 along it), so |scaled score| < 100 here -- the condition holds with two orders of magnitude to spare,
and no case is left out of the comparison.

One batch per S carries every mask kind of the list in _specs (prefix lengths around each 64-key edge, left padding,
holes, holes that end in the first block, an all-zero mask); a second batch runs with mask=None.  S = 64 / 128: the 4- and
8-wave forward and the 32-key-block backward; S = 192: three forward blocks, the odd pass (its backward is the two-kernel
form, unchanged, compared all the same); S = 256: four forward blocks and the 64-key-block backward.  Each with dropout 0
and 0.1: the dropout mask is indexed by position and must not move.

Poison: dqkv is NaN-filled before every backward; the dK / dV rows of the skipped blocks must come back as +0 and no NaN
may survive.  K and V rows past the last unmasked key are overwritten with large finite values: with the switch on the
results must still equal the switch-off results of the clean inputs."""
import math

import numpy as np
import pytest
import torch

from tests import attention_cases as ac
from tests.util import dev

pytestmark = pytest.mark.gpu

A = 2
H = A * 64
SWITCH = "POLUS_ATTN_KSKIP"
BWD_BLOCK = {64: 32, 128: 32, 256: 64}       # key block of the one-pass backward that runs at S


@pytest.fixture(scope="module")
def ops():
    from polus_amd import ops as _ops
    _ops.set_dynamic_params(None)            # the dropout seed as passed (no per-step salt)
    return _ops


def _specs(S):
    lens = [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, S - 1, S]
    specs = []
    for L in lens:
        if 1 <= L <= S and f"len:{L}" not in specs:
            specs.append(f"len:{L}")
    return specs + [f"left:{S // 3 + 1}", "holes", "holes-first", "zero"]


def _mask_row(spec, S, rng):
    if spec == "holes-first":                # holes whose last kept key sits in the first 64-key block
        m = ac.mask_row("holes", S, rng)
        m[40:] = 0
        return m
    return ac.mask_row(spec, S, rng)


def _inputs(S, specs, seed):
    """qkv [B, S, 3H], mask [B, S], dctx [B, S, H]: tests/attention_cases.py make_inputs, for the masks above."""
    r = np.random.Generator(np.random.PCG64(seed))
    B = len(specs)
    qkv = r.standard_normal((B, S, 3 * H)) * 0.7
    dctx = r.standard_normal((B, S, H))
    mask = np.stack([_mask_row(s, S, r) for s in specs])
    u = r.standard_normal((A, 64))
    u = (u / np.linalg.norm(u, axis=1, keepdims=True)).reshape(H)
    qkv[..., :H] += 4.0 * u
    for b in range(B):
        boost = max(0.0, math.log(max(int(mask[b].sum()), 1)) - 1.0)
        for j, key in enumerate(ac.edge_keys(mask[b])):
            if key is not None:
                qkv[b, key, H:2 * H] += 2.0 * boost * u
                qkv[b, key, 2 * H:] = (3.0 + j) * np.where(r.random(H) < 0.5, -1.0, 1.0)
    return qkv, mask, dctx


def _kend(m):
    kept = np.nonzero(m)[0]
    return int(kept[-1]) + 1 if kept.size else m.size


_BATCHES = {}


def _batch(S):
    """Device inputs of the masked batch of S, built once: (qkv, mask, dctx, numpy mask)."""
    if S not in _BATCHES:
        qkv, mask, dctx = _inputs(S, _specs(S), seed=1000 + S)
        B = mask.shape[0]
        _BATCHES[S] = (dev(qkv.reshape(B * S, 3 * H), torch.bfloat16), dev(mask),
                       dev(dctx.reshape(B * S, H), torch.bfloat16), mask)
    return _BATCHES[S]


def _run(ops, on, qkv_t, mask_t, dctx_t, B, S, p, seed=77):
    ops.set_env(SWITCH, 1 if on else 0)
    try:
        ctx = torch.full((B * S, H), float("nan"), dtype=torch.bfloat16, device="cuda")
        lse = torch.full((B, A, S), float("nan"), dtype=torch.float32, device="cuda")
        ops.attention_fwd(qkv_t, mask_t, ctx, lse, B, S, A, drop_p=p, seed=seed)
        dqkv = torch.full((B * S, 3 * H), float("nan"), dtype=torch.bfloat16, device="cuda")
        ops.attention_bwd(qkv_t, mask_t, ctx, dctx_t, lse, dqkv, B, S, A, drop_p=p, seed=seed)
        torch.cuda.synchronize()
    finally:
        ops.set_env(SWITCH)
    return {"ctx": ctx, "lse": lse, "dqkv": dqkv}


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _assert_same_bits(on, off, what):
    for nm in ("ctx", "lse", "dqkv"):
        assert not torch.isnan(on[nm]).any(), f"{what}: NaN left in {nm} (switch on)"
        assert not torch.isnan(off[nm]).any(), f"{what}: NaN left in {nm} (switch off)"
        diff = int((_bits(on[nm]) != _bits(off[nm])).sum())
        assert diff == 0, f"{what}: {nm} differs in {diff} elements between switch on and off"


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", [64, 128, 192, 256])
def test_switch_on_equals_switch_off_bitwise(ops, S, p):
    qkv_t, mask_t, dctx_t, mask = _batch(S)
    B = mask.shape[0]
    on = _run(ops, True, qkv_t, mask_t, dctx_t, B, S, p)
    off = _run(ops, False, qkv_t, mask_t, dctx_t, B, S, p)
    _assert_same_bits(on, off, f"S={S} p={p} masks {'+'.join(_specs(S))}")
    on = _run(ops, True, qkv_t[:2 * S], None, dctx_t[:2 * S], 2, S, p)
    off = _run(ops, False, qkv_t[:2 * S], None, dctx_t[:2 * S], 2, S, p)
    _assert_same_bits(on, off, f"S={S} p={p} mask=None")


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", [64, 128, 256])
def test_skipped_blocks_are_zero_filled_and_never_read(ops, S, p):
    qkv_t, mask_t, dctx_t, mask = _batch(S)
    B = mask.shape[0]
    blk = BWD_BLOCK[S]
    off = _run(ops, False, qkv_t, mask_t, dctx_t, B, S, p)
    on = _run(ops, True, qkv_t, mask_t, dctx_t, B, S, p)
    dkv = _bits(on["dqkv"]).reshape(B, S, 3 * H)[..., H:].cpu().numpy()
    skipped = 0
    for b in range(B):
        row0 = -(-_kend(mask[b]) // blk) * blk                   # first key of the first skipped block
        skipped += S - row0
        assert (dkv[b, row0:] == 0).all(), f"S={S} p={p} sample {b}: dK / dV rows from {row0} on are not all +0"
    assert skipped > 0
    assert not torch.isnan(on["dqkv"]).any(), "NaN left in dqkv"

    # K and V rows past the last unmasked key: large, finite, never part of a result (those that share a block with kept
    # keys are still scored: |q . k| <= 256 |q|_1 < 1.2e4, a scaled score under 2000 -- still far below 10 000)
    r = np.random.Generator(np.random.PCG64(5))
    poisoned = qkv_t.clone().reshape(B, S, 3 * H)
    for b in range(B):
        k = _kend(mask[b])
        if k < S:
            poisoned[b, k:, H:] = dev(256.0 * np.where(r.random((S - k, 2 * H)) < 0.5, -1.0, 1.0), torch.bfloat16)
    on_p = _run(ops, True, poisoned.reshape(B * S, 3 * H), mask_t, dctx_t, B, S, p)
    _assert_same_bits(on_p, off, f"S={S} p={p} poisoned K / V rows past kend")
