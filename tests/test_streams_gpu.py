"""GPU: the ordering between the streams of a training step -- main, the weight-gradient side stream
(BertModel._side, POLUS_OVERLAP_DW) and the in-backward update stream (training._UpdateInBackward) -- bit for bit against
the same step on one stream, on the 5-layer case of tests/stream_cases.py (retire-before-reuse happens, every parity
buffer is written again), with one stream at a time held back for three times the single-stream backward pass
(stream_cases.hold): whatever does not formally wait for the held stream has long run when it starts.

Every reference is the same model, batches and seeds with POLUS_OVERLAP_DW=0 (trainers: POLUS_UPDATE_IN_BACKWARD=0 too);
equal means torch.equal / == on floats.  Test 1 ties that reference to the float64 oracle.  Each held run asserts from
HIP events that the hold lasted as long as asked and, where the main stream has to join the held one, that the main
stream's timed span took at least 0.9 of the hold -- it really waited.  All times are printed with a [streams] prefix."""
import contextlib

import numpy as np
import pytest
import torch

from tests import mlm_ref as mr
from tests import stream_cases as sc
from tests.test_model_gpu import TOLS
from tests.util import assert_close, assert_close_elem, host

pytestmark = pytest.mark.gpu
NAN = float("nan")
STEPS = 6


# ------------------------------------------------------------------------------------------------------------ helpers
def _cfg(dropout):
    from polus_amd.models import BertConfig
    p = 0.1 if dropout else 0.0
    return BertConfig(*sc.CFG_ARGS, hidden_dropout_prob=p, attention_probs_dropout_prob=p)


def _classifier(mode, dropout=True):
    from polus_amd.models import BertModel
    _, params, hw, hb = sc.setup()
    m = BertModel(_cfg(dropout), compute_dtype=mode, num_labels=sc.NUM_LABELS)
    m.load_numpy_params(params, hw, hb)
    m.deterministic = True
    return m


def _switches(monkeypatch, overlap, update_in_backward=None, defer=True):
    monkeypatch.setenv("POLUS_OVERLAP_DW", "1" if overlap else "0")
    if update_in_backward is None:
        monkeypatch.delenv("POLUS_UPDATE_IN_BACKWARD", raising=False)
    else:
        monkeypatch.setenv("POLUS_UPDATE_IN_BACKWARD", "1" if update_in_backward else "0")
    if defer:
        monkeypatch.delenv("POLUS_LN_DEFER_FINALIZE", raising=False)
    else:
        monkeypatch.setenv("POLUS_LN_DEFER_FINALIZE", "0")


def _side_of(m):
    """The side stream of a BertModel, made ahead of its first backward so that there is something to hold."""
    assert m.overlap_dw
    if m._side is None:
        m._side = sc.independent_stream(torch.cuda.current_stream())
    return m._side


def _poison(arena):
    """NaN in every variable's gradient window (the padding between windows stays zero: nothing writes it)."""
    arena.grads.zero_()
    for v in arena.vars:
        v.grad.fill_(NAN)


class Watch:
    """The holds and timed spans of one run; `check` reads the events once the device is idle."""

    def __init__(self, what):
        self.what, self.holds, self.spans = what, [], []

    def hold(self, stream, ms, after=None):
        """`after`: the delay starts no earlier than the point `after` (another stream) has reached now -- so that a span
        timed on `after` from here on contains the whole delay.  The wait is this helper's, not the hold's."""
        if after is not None:
            ev = torch.cuda.Event()
            ev.record(after)
            stream.wait_event(ev)
        h = sc.hold(stream, ms)
        self.holds.append(h)
        return h

    @contextlib.contextmanager
    def span(self, stream, joins=None):
        """Times what `stream` runs inside; `joins` (rec[2], may be set inside): a Hold queued INSIDE the span that this
        work must wait for.  The span opens before the hold is queued, so it contains the hold from its start however
        the two streams map to hardware queues."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rec = [e0, e1, joins]
        self.spans.append(rec)
        yield rec
        e1.record(stream)

    def span_ms(self):
        torch.cuda.synchronize()
        return [e0.elapsed_time(e1) for e0, e1, _ in self.spans]

    def check(self):
        torch.cuda.synchronize()
        got = [(h.ms, h.measured_ms()) for h in self.holds]
        spans = [(e0.elapsed_time(e1), j.ms if j is not None else None) for e0, e1, j in self.spans]
        if got:
            print(f"[streams] {self.what}: {len(got)} hold(s) of {got[0][0]:.1f} ms requested, measured "
                  f"{min(m for _, m in got):.1f} .. {max(m for _, m in got):.1f} ms")
        joined = [(t, ms) for t, ms in spans if ms is not None]
        if joined:
            print(f"[streams] {self.what}: main-stream spans that join a held stream "
                  f"{min(t for t, _ in joined):.1f} .. {max(t for t, _ in joined):.1f} ms")
        # kept for the end of the test (_assert_timing): the comparison of the values speaks first
        for ms, measured in got:
            if not measured >= ms:
                TIMING_FAILURES.append(f"{self.what}: a hold of {ms:.1f} ms lasted {measured:.1f} ms")
        for t, ms in joined:
            if not t >= sc.JOIN_FRACTION * ms:
                TIMING_FAILURES.append(f"{self.what}: the main stream took {t:.1f} ms beside a hold of {ms:.1f} ms: it did not wait")
        return sum(ms for ms, _ in got)


TIMING_FAILURES = []


@pytest.fixture(autouse=True)
def _fresh_timing():
    del TIMING_FAILURES[:]
    yield


def _assert_timing():
    """Every hold of this test lasted as long as asked, and every main-stream span that had to join one took 0.9 of it."""
    assert not TIMING_FAILURES, "; ".join(TIMING_FAILURES)


@pytest.fixture(scope="module", autouse=True)
def _warm():
    """Calibrate the delay and run one step per engine before anything is timed: kernels loaded, workspaces grown."""
    from polus_amd.losses import SparseCategoricalCrossentropy
    sc.calibration()
    for mode in ("f32", "bf16"):
        m = _classifier(mode)
        fn = SparseCategoricalCrossentropy(grad_dtype=m.compute_dtype)
        x, y = sc.inputs(sc.batch(sc.SEEDS[0]))
        for _ in range(2):
            fn(y, m(**x, training=True))
            m.backward(fn.backward())
    torch.cuda.synchronize()
    yield


def _hold_ms(what, backward_ms):
    ms = sc.hold_ms_for(backward_ms)
    print(f"[streams] {what}: single-stream backward {backward_ms:.3f} ms -> holds of {ms:.1f} ms")
    return ms


# ------------------------------------------------------------------------------------- 1. the reference against float64
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_single_stream_gradients_match_the_oracle(mode, monkeypatch):
    """Five layers, one stream, dropout 0: every parameter gradient against ob.token_classifier_bwd in float64, at the
    bounds of tests/test_model_gpu.py::test_forward_backward_matches_golden (per tensor and per element)."""
    from polus_amd.losses import SparseCategoricalCrossentropy
    _switches(monkeypatch, overlap=False)
    m = _classifier(mode, dropout=False)
    assert not m.overlap_dw
    fn = SparseCategoricalCrossentropy(grad_dtype=m.compute_dtype)
    x, y = sc.inputs(sc.batch(sc.SEEDS[0]))
    _poison(m.arena)
    fn(y, m(**x, training=True))
    m.backward(fn.backward())
    torch.cuda.synchronize()
    assert m._side is None and all(l.dw_done is None for l in m.layer)
    ref = sc.oracle_grads(sc.SEEDS[0])
    got = {v.name: host(v.grad) for v in m.trainable_weights}
    assert set(got) == set(ref)
    tol = TOLS[mode]["grad"]
    for k in sorted(ref):
        assert_close(got[k], ref[k], tol, f"grad {k}")
        if mode == "f32":
            assert_close_elem(got[k], ref[k], 5e-4, 5e-4, f"grad {k} (per element)")
        else:
            assert_close_elem(got[k], ref[k], 0.1, 0.2, f"grad {k} (per element)")


# --------------------------------------------------------------------- 2. side-stream backward == single-stream backward
def _backward_run(monkeypatch, mode, accumulate, overlap, defer=True, held=None, hold_ms=0.0, what=""):
    """Forward, loss, backward at model level (twice with `accumulate`, the second pass added to the first on another
    batch).  held: None | "side" (at the start of backward) | "main" (between the loss and backward)."""
    from polus_amd.losses import SparseCategoricalCrossentropy
    _switches(monkeypatch, overlap, defer=defer)
    m = _classifier(mode)
    fn = SparseCategoricalCrossentropy(grad_dtype=m.compute_dtype)
    main = torch.cuda.current_stream()
    w = Watch(what)
    side = _side_of(m) if held else None      # one that does not share a hardware queue with main, whichever is held
    _poison(m.arena)
    losses = []
    for i, seed in enumerate(sc.SEEDS[:2 if accumulate else 1]):
        x, y = sc.inputs(sc.batch(seed))
        losses.append(fn(y, m(**x, training=True)))
        dl = fn.backward()
        if held == "main":
            w.hold(main, hold_ms)
        with w.span(main) as sp:
            sp[2] = w.hold(side, hold_ms, after=main) if held == "side" else None
            m.backward(dl, accumulate=i > 0)
    grads = m.arena.grads.clone()            # on the main stream: whatever follows a backward sees finished gradients
    times = w.span_ms()
    held_total = w.check()
    if overlap:
        assert m._side is not None and all(isinstance(l.dw_done, torch.cuda.Event) for l in m.layer)
    else:
        assert m._side is None and all(l.dw_done is None for l in m.layer)
    return [float(l) for l in losses], grads, max(times), held_total


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_side_stream_backward_equals_single_stream_backward(mode, accumulate, monkeypatch):
    tag = f"backward {mode} {'accumulate' if accumulate else 'overwrite'}"
    l_ref, g_ref, bwd_ms, _ = _backward_run(monkeypatch, mode, accumulate, overlap=False, what=tag + " reference")
    assert not torch.isnan(g_ref).any(), "the reference left a gradient window unwritten"
    ms = _hold_ms(tag, bwd_ms)
    runs = [("overlap on", dict()),
            ("side stream held", dict(held="side")),
            ("main stream held before backward", dict(held="main")),
            ("finalisations on main", dict(defer=False)),
            ("finalisations on main, side stream held", dict(defer=False, held="side"))]
    total = 0.0
    for name, kw in runs:
        l, g, _, held_ms = _backward_run(monkeypatch, mode, accumulate, overlap=True, hold_ms=ms, what=f"{tag}, {name}", **kw)
        total += held_ms
        assert l == l_ref, (name, l, l_ref)
        assert torch.equal(g, g_ref), f"{tag}, {name}: {(g != g_ref).sum().item()} gradient elements differ from the single-stream run"
    print(f"[streams] {tag}: {total:.0f} ms held in all")
    _assert_timing()


# ------------------------------------------------------------ 3. what follows a backward: finished gradients, free buffers
def _plan_run(monkeypatch, overlap, hold_ms=0.0, what=""):
    from polus_amd.losses import SparseCategoricalCrossentropy
    _switches(monkeypatch, overlap)
    m = _classifier("bf16")
    fn = SparseCategoricalCrossentropy(grad_dtype=m.compute_dtype)
    main = torch.cuda.current_stream()
    w = Watch(what)
    side = _side_of(m) if overlap and hold_ms else None
    out, losses, junk = [], [], []
    for s, item in enumerate(sc.PLAN):
        if item[0] == "infer":
            x, _ = sc.inputs(sc.batch(900, item[1], item[2]))
            m(x, training=False)
            continue
        x, y = sc.inputs(sc.batch(700 + s, *item))
        losses.append(fn(y, m(**x, training=True)))
        dl = fn.backward()
        with w.span(main) as sp:
            sp[2] = w.hold(side, hold_ms, after=main) if side is not None else None
            m.backward(dl)
        out.append(m.arena.grads.clone())
        # blocks the shape changes release come back here, poisoned: a late side stream would read them
        junk = [torch.full((1 << 18,), NAN, device=m.arena.device) for _ in range(8)]
    times = w.span_ms()
    w.check()
    del junk
    return [float(l) for l in losses], out, max(times)


def test_what_follows_a_backward_sees_finished_gradients_and_may_reuse_its_buffers(monkeypatch):
    """Changing shapes replace the scratch and activation buffers the side stream reads, an inference call runs in between,
    poisoned allocations take the released blocks, nothing synchronises with the host between the steps (beyond what the
    engine does itself when a workspace grows) -- and the side stream is late in every backward."""
    l_ref, g_ref, bwd_ms = _plan_run(monkeypatch, overlap=False, what="plan reference")
    ms = _hold_ms("plan", bwd_ms)
    l, g, _ = _plan_run(monkeypatch, overlap=True, hold_ms=ms, what="plan, side stream held in every backward")
    assert l == l_ref, (l, l_ref)
    assert len(g) == len(g_ref) == sum(1 for p in sc.PLAN if p[0] != "infer")
    for s, (a, b) in enumerate(zip(g, g_ref)):
        assert not torch.isnan(b).any()
        assert torch.equal(a, b), f"training step {s} of the plan: {(a != b).sum().item()} gradient elements differ"
    _assert_timing()


# ----------------------------------------------------------------------------------------------- 4. tied masked-LM head
def _mlm_run(monkeypatch, mode, overlap, hold_ms=0.0, what=""):
    from polus_amd.losses import MaskedSparseCategoricalCrossentropy
    from polus_amd.models import BertForMaskedLM
    _switches(monkeypatch, overlap)
    ocfg = sc.setup()[0]
    m = BertForMaskedLM(_cfg(True), compute_dtype=mode)
    m.load_numpy_params(mr.mlm_params(ocfg))
    m.deterministic = True
    fn = MaskedSparseCategoricalCrossentropy()
    main = torch.cuda.current_stream()
    w = Watch(what)
    side = _side_of(m.bert) if overlap and hold_ms else None
    _poison(m.arena)
    losses, out = [], []
    for i, seed in enumerate((31, 32)):                 # the second pass is added to the first: both forms of the tied share
        ids, mask, tt, pos, lab = mr.mlm_batch(ocfg, sc.B, sc.S, 6, seed)
        logits = m(input_ids=ids, attention_mask=mask, token_type_ids=tt, masked_positions=pos, training=True)
        losses.append(fn(lab, logits))
        dl = fn.backward()
        with w.span(main) as sp:
            sp[2] = w.hold(side, hold_ms, after=main) if side is not None else None
            m.backward(dl, accumulate=i > 0)
        out.append(m.arena.grads.clone())
    times = w.span_ms()
    w.check()
    assert (m.bert._side is not None) == overlap
    return [float(l) for l in losses], out, max(times)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_tied_masked_lm_head_with_the_side_stream(mode, monkeypatch):
    """emb.word's window takes the decoder's share, then the embedding backward's, while the layers' weight gradients are
    still on the side stream; only then is it final."""
    l_ref, g_ref, bwd_ms = _mlm_run(monkeypatch, mode, overlap=False, what=f"mlm {mode} reference")
    ms = _hold_ms(f"mlm {mode}", bwd_ms)
    for name, hold in (("overlap on", 0.0), ("side stream held", ms)):
        l, g, _ = _mlm_run(monkeypatch, mode, overlap=True, hold_ms=hold, what=f"mlm {mode}, {name}")
        assert l == l_ref, (name, l, l_ref)
        for a, b in zip(g, g_ref):
            assert not torch.isnan(b).any()
            assert torch.equal(a, b), f"mlm {mode}, {name}: {(a != b).sum().item()} gradient elements differ"
    _assert_timing()


# -------------------------------------------------------------------------------------------------------- 5. split model
def _split_run(monkeypatch, overlap, hold_ms=0.0, what=""):
    from polus_amd.models import BertModel, split_bert_model
    _switches(monkeypatch, overlap)
    ocfg, params, _, _ = sc.setup()
    full = BertModel(_cfg(True), compute_dtype="bf16")
    full.load_numpy_params(params)
    pre, post = split_bert_model(full, 2)
    assert len(pre.layer) == 2 and [l.index for l in post.layer] == [2, 3, 4]
    pre.deterministic = post.deterministic = True
    ids, mask, tt, _ = sc.batch(sc.SEEDS[0])
    H = ocfg.hidden_size
    dy = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).standard_normal((sc.B, sc.S, H)).astype(np.float32) * 0.1)
    dy = dy.to(torch.bfloat16).cuda()
    main = torch.cuda.current_stream()
    w = Watch(what)
    # every half that can overlap gets its side stream held (a half without one runs its backward on the main stream)
    sides = [_side_of(h) for h in (pre, post) if overlap and hold_ms and getattr(h, "overlap_dw", False)]
    _poison(pre.arena)
    hs = pre(input_ids=ids, attention_mask=mask, token_type_ids=tt, training=True).last_hidden_state
    post(hidden_states=hs, attention_mask=mask, training=True)
    with w.span(main) as sp:
        holds = [w.hold(s, hold_ms, after=main) for s in sides]
        sp[2] = holds[0] if holds else None
        dx = post.backward(dy)
        dx_kept = dx.clone()
        pre.backward(dx)                      # a view of the upper half's scratch, consumed by the lower half
    grads = pre.arena.grads.clone()
    times = w.span_ms()
    w.check()
    assert (pre._side is not None) == overlap
    return grads, dx_kept, max(times)


def test_split_model_with_the_side_stream(monkeypatch):
    g_ref, dx_ref, bwd_ms = _split_run(monkeypatch, overlap=False, what="split reference")
    assert not torch.isnan(g_ref).any() and not torch.isnan(dx_ref.float()).any()
    ms = _hold_ms("split", bwd_ms)
    for name, hold in (("overlap on", 0.0), ("side streams held", ms)):
        g, dx, _ = _split_run(monkeypatch, overlap=True, hold_ms=hold, what=f"split, {name}")
        assert torch.equal(dx, dx_ref), f"split, {name}: the gradient handed from the upper to the lower half differs"
        assert torch.equal(g, g_ref), f"split, {name}: {(g != g_ref).sum().item()} gradient elements differ"
    _assert_timing()


# ------------------------------------------------------------------------------------------ 6./7. trainer, three streams
def _marked_loss(grad_dtype):
    from polus_amd.losses import SparseCategoricalCrossentropy

    class MarkedLoss(SparseCategoricalCrossentropy):
        """`before_backward()` runs on entry of backward(): the point between the loss and the model's backward pass."""
        before_backward = None

        def backward(self, accumulate=False):
            if self.before_backward is not None:
                self.before_backward()
            return super().backward(accumulate)
    return MarkedLoss(grad_dtype=grad_dtype)


def _trainer_run(monkeypatch, mode, accum, on, held=None, hold_ms=0.0, stream=None, what=""):
    """6 optimizer steps (x accum micro-steps).  on: both overlaps (the update forced: 144 tokens are below the size rule);
    held: None | "side" | "update" (at the start of every train_step) | "main" (at the start of backward)."""
    from polus_amd.optimizers import AdamWeightDecay
    from polus_amd.schedulers import warmup_scheduler
    from polus_amd.training import ClassifierTrainer
    _switches(monkeypatch, overlap=on, update_in_backward=on)
    m = _classifier(mode)
    loss = _marked_loss(m.compute_dtype)
    t = ClassifierTrainer(m, AdamWeightDecay(learning_rate=warmup_scheduler(STEPS, 1e-3), weight_decay_rate=0.01), loss)
    t.grad_accum_steps = accum
    updater = t._updater()
    assert (updater is not None) == on
    torch.cuda.synchronize()                  # the parameters were loaded on the default stream
    w = Watch(what)
    backward_ms = []
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        main = torch.cuda.current_stream()
        assert stream is None or main == stream
        target = None
        if held is not None:
            # streams a hold of one leaves running (see stream_cases.blocks); the updater's own is replaced before its first use
            side = _side_of(m)
            updater.stream = sc.independent_stream(main, side)
            target = {"side": side, "update": updater.stream}.get(held)
        marks = []
        if held == "main":
            loss.before_backward = lambda: w.hold(torch.cuda.current_stream(), hold_ms)
        elif not on:
            def mark():                       # the single-stream backward (and update) time that sizes the holds
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(torch.cuda.current_stream())
                marks.append(ev)
            loss.before_backward = mark
        losses, ends = [], []
        for s in range(STEPS * accum):
            ids, mask, tt, labels = sc.batch(700 + s)
            x = {k: torch.tensor(v).cuda() for k, v in (("input_ids", ids), ("attention_mask", mask), ("token_type_ids", tt))}
            y = torch.tensor(labels).cuda()          # made on the stream the step runs on
            with w.span(main) as sp:
                h = w.hold(target, hold_ms, after=main) if target is not None else None
                # the update stream is joined by the micro-step that completes an accumulation; the side stream by every one
                sp[2] = h if (held == "side" or s % accum == accum - 1) else None
                losses.append(t.train_step(x, y))
            if not on:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(main)
                ends.append(ev)
        out = [float(l) for l in losses]      # read late: nothing waited for the GPU between the steps
        torch.cuda.synchronize()
        w.check()
        assert t._updater() is updater and t.optimizer.iterations == STEPS
        if on:
            assert m._side is not None and all(isinstance(l.dw_done, torch.cuda.Event) for l in m.layer)
        mm, vv = t.optimizer._slots(m.arena)
        state = {"params": m.arena.params.clone(), "m": mm.clone(), "v": vv.clone()}
        if m.arena.shadow is not None:
            state["shadow"] = m.arena.shadow.clone()
        if m.arena.shadow_t is not None:
            state["shadow_t"] = m.arena.shadow_t.clone()
        torch.cuda.synchronize()
    if marks:
        backward_ms = [a.elapsed_time(b) for a, b in zip(marks, ends)]
    return out, state, (max(backward_ms[1:]) if backward_ms else None)


def _same_training(tag, name, got, ref):
    (l, s), (l_ref, s_ref) = got, ref
    assert l == l_ref, (tag, name, l, l_ref)
    assert set(s) == set(s_ref)
    for k in s_ref:
        assert torch.equal(s[k], s_ref[k]), f"{tag}, {name}: {(s[k] != s_ref[k]).sum().item()} elements of {k} differ"


@pytest.mark.parametrize("accum", [1, 2])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_trainer_on_three_streams_equals_one_stream(mode, accum, monkeypatch):
    """Side-stream weight gradients and the in-backward AdamW together, each of the three streams late in turn.  With the
    update stream held the next step's forward must still read updated parameters and refreshed transposed shadows."""
    tag = f"trainer {mode} accum {accum}"
    l_ref, s_ref, bwd_ms = _trainer_run(monkeypatch, mode, accum, on=False, what=tag + " reference")
    assert ("shadow_t" in s_ref) == (mode == "bf16")
    ms = _hold_ms(tag, bwd_ms)
    for name, held in (("no hold", None), ("side stream held", "side"), ("update stream held", "update"),
                       ("main stream held before backward", "main")):
        l, s, _ = _trainer_run(monkeypatch, mode, accum, on=True, held=held, hold_ms=ms, what=f"{tag}, {name}")
        _same_training(tag, name, (l, s), (l_ref, s_ref))
    _assert_timing()


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_trainer_under_a_user_stream_equals_the_default_stream(mode, monkeypatch):
    """`with torch.cuda.stream(s)`: the step pins s; the events the side and update streams wait on must be recorded on
    the stream the kernels were launched on."""
    tag = f"trainer {mode} under a user stream"
    ref = _trainer_run(monkeypatch, mode, 1, on=False, what=tag + ": reference")[:2]
    default = _trainer_run(monkeypatch, mode, 1, on=True, what=tag + ": default stream")[:2]
    s = torch.cuda.Stream()
    assert s != torch.cuda.current_stream()
    user = _trainer_run(monkeypatch, mode, 1, on=True, stream=s, what=tag)[:2]
    _same_training(tag, "default stream against the single-stream reference", default, ref)
    _same_training(tag, "user stream against the default stream", user, default)
