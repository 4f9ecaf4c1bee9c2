"""The case of tests/stream_cases.py, checked without a GPU: a bitwise comparison of two runs of it can only expose a
misplaced event wait if the values a stale or mixed-up buffer would deliver differ from the right ones."""
import numpy as np
import pytest

from tests import stream_cases as sc


def test_the_case_reuses_each_parity_buffer_twice_and_unevenly():
    L = sc.CFG_ARGS[2]
    assert L >= 5 and L % 2 == 1
    order = list(reversed(range(L)))                      # the order backward visits the layers in
    per_parity = {p: [k for k in order if k & 1 == p] for p in (0, 1)}
    assert len(per_parity[0]) - 1 >= 2                    # a buffer set written again at least twice
    assert len(per_parity[0]) != len(per_parity[1])
    assert sum(1 for i in range(L) if i >= 2) >= 3        # `len(pending) == 2` holds inside the loop at least three times


def test_every_oracle_gradient_is_non_zero():
    g = sc.oracle_grads()
    ocfg = sc.setup()[0]
    assert len(g) == 5 + 12 * ocfg.num_hidden_layers + 2
    for k, a in g.items():
        assert np.isfinite(a).all() and np.abs(a).max() > 0, k
        # no window is a few stray entries: a stale tile must change something.  (The tables only get the rows the batch
        # touches; the key third of qkv.b has a gradient of zero by the softmax's shift invariance, a few entries exactly.)
        if k not in ("emb.word", "emb.pos", "emb.type"):
            assert (a != 0).mean() > 0.9, k


def test_gradients_two_layers_apart_differ():
    """Layers k and k + 2 share the dY buffers of one parity.  If one read the other's, or a stale one, the gradients
    would be the other layer's: they must not be (nearly) equal to begin with -- judged at the coarsest precision the
    engine stores anything in, bf16 (2^-8 relative)."""
    g = sc.oracle_grads()
    L = sc.setup()[0].num_hidden_layers
    for k in range(L - 2):
        keys = sc.layer_keys(g, k)
        assert keys == sc.layer_keys(g, k + 2) and len(keys) == 12
        for name in keys:
            a, b = g[f"layer{k}.{name}"], g[f"layer{k + 2}.{name}"]
            scale = max(np.abs(a).max(), np.abs(b).max())
            far = np.abs(a - b) > 2.0 ** -6 * scale
            assert far.mean() > 0.25, (k, name, far.mean())


def test_the_two_micro_batches_give_different_gradients():
    a, b = sc.oracle_grads(sc.SEEDS[0]), sc.oracle_grads(sc.SEEDS[1])
    assert not np.array_equal(sc.batch(sc.SEEDS[0])[0], sc.batch(sc.SEEDS[1])[0])
    for k in a:
        scale = max(np.abs(a[k]).max(), np.abs(b[k]).max())
        assert (np.abs(a[k] - b[k]) > 2.0 ** -6 * scale).any(), k


def test_plan_changes_shape_both_ways_around_an_inference_call():
    train = [p for p in sc.PLAN if p[0] != "infer"]
    tokens = [b * s for b, s in train]
    assert any(y < x for x, y in zip(tokens, tokens[1:])) and any(y > x for x, y in zip(tokens, tokens[1:]))
    assert max(s for _, s in train) <= sc.CFG_ARGS[5] and sum(1 for p in sc.PLAN if p[0] == "infer") == 1
    assert train[0] == train[-1] == (sc.B, sc.S)


@pytest.mark.parametrize("backward_ms,expect", [(0.0, 20.0), (2.0, 20.0), (6.0, 20.0), (20.0 / 3.0, 20.0), (7.0, 21.0),
                                                (50.0, 150.0), (83.0, 249.0), (84.0, 250.0), (1000.0, 250.0)])
def test_hold_length_rule(backward_ms, expect):
    assert sc.hold_ms_for(backward_ms) == pytest.approx(expect, abs=1e-12)


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_hold_length_rule_rejects_what_is_no_time(bad):
    with pytest.raises(ValueError):
        sc.hold_ms_for(bad)
