"""CPU test doubles for the host-logic tests: a tiny NumPy softmax-regression 'model' that
implements the model / loss / optimizer protocols the trainer drives (the oracle is the
compute here — test infrastructure only), and a recording proxy over the real library for the
wrapper-contract tests."""
import numpy as np
import torch

from oracle import losses as ol
from polus_amd.optimizers import _LearningRate


class RecordingLib:
    """A proxy over the real in-tree library for the wrapper-contract tests: the host-only functions (workspace sizes, route
    reports, polus_last_error, polus_abi_version, ...) go to the real library; every other entry point is recorded as
    (name, args) and answers POLUS_OK without touching the device."""
    HOST_ONLY = ("_workspace_bytes", "_route", "_supported")
    HOST_ONLY_NAMES = ("polus_last_error", "polus_abi_version")

    def __init__(self, real):
        self._real = real
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("polus_"):
            raise AttributeError(name)
        if name.endswith(self.HOST_ONLY) or name in self.HOST_ONLY_NAMES:
            return getattr(self._real, name)
        getattr(self._real, name)                  # an entry point the library does not have is an error here too

        def record(*args):
            self.calls.append((name, args))
            return 0
        return record

    def names(self):
        return [n for n, _ in self.calls]


def recording_lib(real, monkeypatch, stream):
    """A generator for a fixture to `yield from`: the recording library installed over `real`, the dummy `stream` handle cached
    (so ops._st() needs no device), fresh workspaces; the cached handle is put back afterwards."""
    from polus_amd import _lib, ops
    proxy = RecordingLib(real)
    monkeypatch.setattr(_lib, "load", lambda: proxy)
    monkeypatch.setattr(ops, "_WS", {})
    monkeypatch.setattr(ops, "_HAS_GPU", False)
    prev = _lib._CUR_STREAM[0]
    _lib._CUR_STREAM[0] = stream
    try:
        yield proxy
    finally:
        _lib._CUR_STREAM[0] = prev


def disable_device_check(monkeypatch):
    """Let the wrappers of polus_amd.ops take CPU tensors: for runs against the recording library only."""
    from polus_amd import ops
    monkeypatch.setattr(ops, "_req_cuda", lambda *ts: None)


class FakeArena:
    def __init__(self, n):
        self.grads = torch.zeros(n, dtype=torch.float32)
        self.params = torch.zeros(n, dtype=torch.float32)
        self.shadow = None
        self.vars = []

    def refresh_shadow(self, var=None):
        pass


class FakeVar:
    def __init__(self, arena, name, offset, shape):
        self.arena, self.name, self.offset, self.shape = arena, name, offset, shape
        self.size = int(np.prod(shape))

    @property
    def value(self):
        return self.arena.params[self.offset:self.offset + self.size].view(self.shape)

    @property
    def grad(self):
        return self.arena.grads[self.offset:self.offset + self.size].view(self.shape)


class FakeLinearModel:
    """logits = x W^T + b with NumPy math; grads land in a flat CPU 'arena'."""
    name = "fake"

    def __init__(self, n_in=5, n_out=3, seed=0):
        self.arena = FakeArena(n_in * n_out + n_out)
        self.w = FakeVar(self.arena, "w", 0, (n_out, n_in))
        self.b = FakeVar(self.arena, "b", n_in * n_out, (n_out,))
        self.arena.vars = [self.w, self.b]
        self.arena.params[:n_in * n_out] = torch.from_numpy(
            np.random.default_rng(seed).standard_normal(n_in * n_out).astype(np.float32))
        self.trainable_weights = [self.w, self.b]
        self.grad_ready_hook = None
        self.calls = []

    def __call__(self, x, training=False):
        self.calls.append(("call", training))
        self._x = np.asarray(x, np.float64)
        return self._x @ self.w.value.numpy().astype(np.float64).T + self.b.value.numpy()

    def backward(self, dlogits, accumulate=False):
        gw = torch.from_numpy((dlogits.T @ self._x).astype(np.float32))
        gb = torch.from_numpy(dlogits.sum(0).astype(np.float32))
        if accumulate:
            self.w.grad.add_(gw); self.b.grad.add_(gb)
        else:
            self.w.grad.copy_(gw); self.b.grad.copy_(gb)
        if self.grad_ready_hook:
            self.grad_ready_hook(self.b.offset, self.b.offset + self.b.size)
            self.grad_ready_hook(self.w.offset, self.w.offset + self.w.size)

    def inference(self, x):
        return np.argmax(self(x), -1).astype(np.int32)

    def save(self, **kw):
        self.calls.append(("save", kw))


class FakeXent:
    def __call__(self, y, logits):
        self.loss, self.d = ol.sparse_softmax_xent_fwd(np.asarray(logits, np.float64), np.asarray(y))
        return float(self.loss)

    def backward(self, accumulate=False):
        return self.d


class FakeSGD:
    def __init__(self, lr=0.1):
        self.learning_rate = _LearningRate(lr)
        self.grad_scale = 1.0
        self.steps = 0

    def variables(self):
        return []

    def apply_gradients(self, grads_and_vars):
        lr = self.learning_rate(self.steps)
        self.steps += 1
        for g, v in grads_and_vars:
            v.value.sub_(lr * self.grad_scale * g)
