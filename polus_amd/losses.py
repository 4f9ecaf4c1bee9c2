"""Loss objects of the Polus step: ``loss(*forward_with_grads_outputs) -> scalar``
(polus/training.py:180) plus ``backward()`` -> gradient wrt the logits, both one HIP launch.

polus/losses.py:5-41 and the Keras SparseCategoricalCrossentropy(from_logits=True) of
tutorials/classifier_example.py:55.
"""
import numpy as np
import torch

from . import ops
from .tensor import DeviceScalar, to_device


class _XentBase:
    RING = 256

    def __init__(self, grad_dtype=None):
        self.grad_dtype = grad_dtype
        self._bufs = {}

    def _out(self, logits):
        l2 = logits.reshape(-1, logits.shape[-1])
        if l2.dtype != torch.float32:
            l2 = l2.float()
        l2 = l2.contiguous()
        gd = self.grad_dtype or torch.float32
        key = (tuple(l2.shape), gd)
        if self._bufs.get("key") != key:
            self._bufs = {"key": key, "d": torch.empty(l2.shape, dtype=gd, device=l2.device),
                          "ring": torch.empty(self.RING, dtype=torch.float32, device=l2.device), "k": 0}
        # every call hands out its own scalar: a loss kept from step k still reads step k's value after later
        # steps (the reference returns independent tf tensors); the ring wraps after RING steps
        k = self._bufs["k"]
        self._bufs["k"] = (k + 1) % self.RING
        return l2, self._bufs["d"], self._bufs["ring"][k:k + 1]

    def backward(self, accumulate=False):
        return self._dlogits


class SparseCategoricalCrossentropy(_XentBase):
    """mean over every leading dim of -log softmax(logits)[label]."""

    def __init__(self, from_logits=True, grad_dtype=None):
        assert from_logits, "only from_logits=True is on the reference's path"
        super().__init__(grad_dtype)

    def __call__(self, y_true, y_pred):
        l2, d, loss = self._out(y_pred)
        labels = to_device(y_true, torch.int32, l2.device).reshape(-1)
        ops.softmax_xent(l2, labels, loss, d)
        self._dlogits = d.view(y_pred.shape)
        return DeviceScalar(loss)


class MaskedSparseCategoricalCrossentropy(_XentBase):
    """Mean of -log softmax(logits)[label] over the rows whose label is >= 0; rows with a negative label (-1, or the -100
    of HF's CrossEntropyLoss) are left out of the mean and get a zero gradient row.  The masked-LM objective: one
    workgroup per row over a vocabulary-wide class axis (polus_softmax_xent_wide).

    Logits are f32 or bf16 of any leading shape; the last axis must be contiguous and may sit in a padded buffer
    (a row stride that is a multiple of 16 bytes lets the kernel move 16 bytes per lane).  The gradient has the
    logits' dtype and is written IN PLACE over the logits unless `in_place=False`: at 2560 x 30522 the matrix is
    157 MB in bf16.  `counted` / `rejected` are device int32 scalars of the last call: rows that entered the mean, and
    rows whose label was >= the class count (ignored as well; a caller that cares reads it, nothing synchronises here).

    A few classes over many rows (a token classifier with padded labels) works through the same kernel but is not tuned
    for it: a workgroup of 1024 lanes per row of a few dozen classes is mostly idle."""

    def __init__(self, from_logits=True, grad_dtype=None, in_place=True):
        assert from_logits, "only from_logits=True is on the reference's path"
        super().__init__(grad_dtype)
        self.in_place = in_place

    @staticmethod
    def _rows(logits):
        """[rows, V] view with one row stride of a tensor whose leading axes collapse; a contiguous copy otherwise."""
        V = logits.shape[-1]
        if logits.dim() == 1:
            return logits.view(1, V)
        st, sh = logits.stride(), logits.shape
        ok = (st[-1] == 1 or V == 1) and all(st[k] == st[k + 1] * sh[k + 1] for k in range(logits.dim() - 2))
        if not ok:
            logits = logits.contiguous()
            st = logits.stride()
        return logits.as_strided((logits.numel() // V, V), (st[-2], 1))

    def __call__(self, y_true, y_pred):
        if y_pred.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"MaskedSparseCategoricalCrossentropy: f32 or bf16 logits, got {y_pred.dtype}")
        if self.grad_dtype is not None and self.grad_dtype != y_pred.dtype:
            raise TypeError("MaskedSparseCategoricalCrossentropy: the gradient has the logits' dtype "
                            f"({y_pred.dtype}), grad_dtype={self.grad_dtype} asks for another")
        l2 = self._rows(y_pred)
        rows, V = l2.shape
        key = (rows, V, l2.dtype, l2.device)
        if self._bufs.get("key") != key:
            self._bufs = {"key": key, "k": 0, "ring": torch.empty(self.RING, dtype=torch.float32, device=l2.device),
                          "stats": torch.zeros(2, dtype=torch.int32, device=l2.device), "d": None}
        bb = self._bufs
        k = bb["k"]
        bb["k"] = (k + 1) % self.RING
        loss = bb["ring"][k:k + 1]
        labels = to_device(y_true, torch.int32, l2.device).reshape(-1)
        assert labels.numel() == rows, f"{labels.numel()} labels for {rows} rows of logits"
        if self.in_place:
            d = l2
        else:
            if bb["d"] is None:
                ld = (V * l2.element_size() + 15) // 16 * 16 // l2.element_size()      # rows on 16-byte boundaries
                bb["d"] = torch.empty((rows, ld), dtype=l2.dtype, device=l2.device)[:, :V]
            d = bb["d"]
        ops.softmax_xent_wide(l2, labels, loss, d, stats=bb["stats"])
        lead = tuple(y_pred.shape[:-1])
        self._dlogits = d.as_strided(lead + (V,), tuple(d.stride(0) * int(np.prod(lead[j + 1:], dtype=np.int64)) for j in range(len(lead))) + (1,))
        return DeviceScalar(loss)

    @property
    def counted(self):
        return self._bufs["stats"][0]

    @property
    def rejected(self):
        return self._bufs["stats"][1]


def weighted_softmax_cross_entropy_from_logits(class_weights, grad_dtype=None):
    """polus/losses.py:5-18; y_true one-hot."""
    cw_host = np.asarray(class_weights, np.float32)

    class _Loss(_XentBase):
        def __call__(self, y_true, y_pred):
            l2, d, loss = self._out(y_pred)
            yt = to_device(y_true, None, l2.device)
            labels = yt.reshape(-1, yt.shape[-1]).argmax(-1).to(torch.int32).contiguous()
            cw = to_device(cw_host, torch.float32, l2.device)
            ops.softmax_xent(l2, labels, loss, d, class_weights=cw)
            self._dlogits = d.view(y_pred.shape)
            return DeviceScalar(loss)
    return _Loss(grad_dtype)


def weighted_sigmoid_cross_entropy_from_logits(class_weights, negative_weight, grad_dtype=None):
    """polus/losses.py:21-41; y_true multi-hot."""
    cw_host = np.asarray(class_weights, np.float32)

    class _Loss(_XentBase):
        def __call__(self, y_true, y_pred):
            l2, d, loss = self._out(y_pred)
            yt = to_device(y_true, torch.float32, l2.device).reshape(l2.shape)
            cw = to_device(cw_host, torch.float32, l2.device)
            ops.sigmoid_xent(l2, yt, cw, negative_weight, loss, d)
            self._dlogits = d.view(y_pred.shape)
            return DeviceScalar(loss)
    return _Loss(grad_dtype)
