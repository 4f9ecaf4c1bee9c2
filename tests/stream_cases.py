"""The case of the stream-ordering tests, shared by test_stream_cases_cpu.py (is a bitwise comparison of this case able to
fail?) and test_streams_gpu.py, and the one tool those tests need: a bounded delay on one stream.

The case: bert_small with FIVE layers.  BertModel.backward retires a layer's weight-gradient launch two layers later
(`if len(pending) == 2`) and double-buffers the dY tensors that launch reads by layer parity; with an odd count >= 5 each
parity buffer is written again twice (layers 4, 2, 0 share one set) and the two parities are used unevenly (3 and 2).
Parameters are oracle.bert.golden_setup's, batches tests.golden.make_golden.synth_batch's: no golden file.

`hold(stream, ms)` keeps one stream busy for at least `ms` milliseconds with torch.cuda._sleep (a spinning kernel), sized by
a calibration measured with HIP events once per process.  It ends by itself: it waits on no flag, stream or memory.  At
test shapes a side stream's work is done microseconds after it was queued, so a missing event wait never shows; with one
stream held back for three times as long as the whole single-stream backward pass, every other stream has run everything
that does not formally depend on the held one before it starts."""
import functools
import math

CFG_ARGS = (96, 128, 5, 2, 256, 64, 2)       # vocab, hidden, LAYERS, heads, intermediate, max positions, token types
NUM_LABELS = 4
B, S = 3, 48
SEEDS = (1200, 1201)                          # the micro-batches of the `accumulate` variants
# what follows a backward (test 3): training shapes, one inference call in between
PLAN = ((3, 48), (3, 48), (2, 32), (3, 48), ("infer", 4, 40), (5, 64), (3, 48))

HOLD_MIN_MS, HOLD_FACTOR, HOLD_CAP_MS = 20.0, 3.0, 250.0
JOIN_FRACTION = 0.9                           # a stream that joins a held one is busy for at least this much of the hold
# cycles are requested 25 % above the calibrated rate: the spinning kernel counts shader clocks, and the clock of a busy
# device may be above the one the calibration (the same kernel alone on the device) saw
SLEEP_MARGIN = 1.25


def hold_ms_for(backward_ms):
    """Length of a hold for a case whose single-stream backward pass takes `backward_ms`: three times that, at least
    20 ms, at most 250 ms."""
    if not (backward_ms >= 0.0 and math.isfinite(backward_ms)):
        raise ValueError(f"backward time must be a finite, non-negative number of milliseconds, got {backward_ms!r}")
    return min(HOLD_CAP_MS, max(HOLD_MIN_MS, HOLD_FACTOR * backward_ms))


@functools.lru_cache(maxsize=None)
def setup():
    """(oracle config, params, head_w, head_b) in float64; shared, not to be written to."""
    from oracle import bert as ob
    ocfg = ob.BertConfig(*CFG_ARGS)
    params, hw, hb = ob.golden_setup(ocfg, NUM_LABELS)
    return ocfg, params, hw, hb


@functools.lru_cache(maxsize=None)
def batch(seed, b=B, s=S):
    """(ids, mask, token types, labels) of synth_batch: ragged lengths, padded tail; shared, not to be written to."""
    from tests.golden.make_golden import synth_batch
    return synth_batch(setup()[0], b, s, NUM_LABELS, seed)


def inputs(bt):
    ids, mask, tt, labels = bt
    return {"input_ids": ids, "attention_mask": mask, "token_type_ids": tt}, labels


@functools.lru_cache(maxsize=None)
def oracle_grads(seed=SEEDS[0]):
    """Every parameter gradient of the 5-layer token classifier on batch(seed), float64, dropout 0.  Computed once."""
    from oracle import bert as ob
    ocfg, params, hw, hb = setup()
    ids, mask, tt, labels = batch(seed)
    _, _, cache = ob.token_classifier_fwd(params, ocfg, hw, hb, ids, mask, labels, tt)
    g = ob.token_classifier_bwd(params, ocfg, hw, cache)
    for a in g.values():
        a.setflags(write=False)
    return g


def layer_keys(grads, k):
    p = f"layer{k}."
    return sorted(n[len(p):] for n in grads if n.startswith(p))


# ------------------------------------------------------------------------------------------------ holding a stream back
_CAL = {}


def _calibrate_sleep(torch):
    """Cycles of torch.cuda._sleep per millisecond, measured: the request is doubled until one call lasts 5 ms (launch and
    event overhead are then below a percent), then the fastest of three timings counts (most cycles per ms: a hold sized by
    it is the longest)."""
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(cycles):
        e0.record(st)
        torch.cuda._sleep(cycles)
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)
    cycles = 1 << 20
    timed(cycles)                             # the first launch loads the kernel
    while timed(cycles) < 5.0:
        cycles *= 2
        if cycles > 1 << 36:
            raise RuntimeError("torch.cuda._sleep does not last: 2^36 cycles took under 5 ms")
    return max(cycles / timed(cycles) for _ in range(3))


def _calibrate_gemm(torch):
    """Milliseconds of one 1024^3 f32 torch GEMM (the fall-back delay where _sleep is absent)."""
    a = torch.ones((1024, 1024), device="cuda")
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.mm(a, a)
    best = float("inf")
    for _ in range(3):
        e0.record(st)
        for _ in range(16):
            torch.mm(a, a)
        e1.record(st)
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / 16)
    return best, a


def calibration():
    """{"kind": "sleep", "cycles_per_ms": r} or {"kind": "gemm", "ms_per_gemm": t}; measured once per process."""
    if not _CAL:
        import torch
        if hasattr(torch.cuda, "_sleep"):
            _CAL.update(kind="sleep", cycles_per_ms=_calibrate_sleep(torch))
        else:
            t, a = _calibrate_gemm(torch)
            _CAL.update(kind="gemm", ms_per_gemm=t, operand=a)
        print("[streams] calibration: " + ", ".join(f"{k} = {v}" for k, v in _CAL.items() if k != "operand"))
    return _CAL


class Hold:
    """One queued delay: the stream, the length asked for, and timing events right before and behind it."""

    def __init__(self, stream, ms, e0, e1):
        self.stream, self.ms, self.e0, self.e1 = stream, ms, e0, e1

    def measured_ms(self):
        """After the stream has been synchronised.  Events on one stream: the time between them is the delay's own."""
        return self.e0.elapsed_time(self.e1)


def hold(stream, ms):
    """Queue a delay of at least `ms` milliseconds on `stream`; nothing else is queued and no other stream is touched."""
    import torch
    cal = calibration()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        if cal["kind"] == "sleep":
            e0.record(stream)
            torch.cuda._sleep(int(ms * cal["cycles_per_ms"] * SLEEP_MARGIN))
        else:
            a = cal["operand"]                # written and synchronised by the calibration: only read here
            out = torch.empty_like(a)
            e0.record(stream)
            for _ in range(int(math.ceil(ms / cal["ms_per_gemm"] * SLEEP_MARGIN))):
                torch.mm(a, a, out=out)
        e1.record(stream)
    return Hold(stream, ms, e0, e1)


def blocks(stream, other, ms=2.0):
    """Does a delay on `stream` keep `other` from running?  Streams are spread over a few hardware queues; two that share
    one run in the order they were fed, so work queued on `other` behind a hold of `stream` starts after it whether or
    not anything orders the two -- a held run on such a pair cannot show a missing wait.  Measured: a marker on `other`
    before a short hold of `stream`, one behind it."""
    import torch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(other)
    hold(stream, ms)
    e1.record(other)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) >= 0.5 * ms


def independent_stream(*others, tries=8):
    """A new stream whose holds leave `others` running, if `tries` new streams hold one; the last one made otherwise
    (the tests then still compare, the held runs just cannot expose anything on that pair)."""
    import torch
    for k in range(tries):
        st = torch.cuda.Stream()
        shared = [o for o in others if blocks(st, o)]
        if not shared:
            return st
        print(f"[streams] new stream {k} shares a hardware queue with {len(shared)} of the streams it must run beside: next")
    print(f"[streams] no independent stream among {tries}: held runs on this one are not sensitive")
    return st
