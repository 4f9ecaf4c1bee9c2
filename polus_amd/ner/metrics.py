"""polus/ner/metrics.py drop-in: EntityF1, the strict entity-level micro F1 that NER checkpoints are selected by, plus
MacroF1Score / Accuracy (the reference's sequential versions differ from polus/metrics.py only in flattening [B, S],
which polus_amd.metrics already does).

Two device tensors are counted where they are -- one polus_bio_entity_counts launch per batch into int32 accumulators in
HBM, no device-to-host copy per validation step -- and only the [T, 3] counts come to the host in evaluate(); host
arrays (the gathered tuples of other ranks) are counted in NumPy by polus_amd.ner.bio.entity_counts."""
import numpy as np

from ..context import logger
from ..metrics import Accuracy, IMetric, MacroF1Score, _divide_no_nan  # noqa: F401  (re-exported)
from . import bio

_DEV_MAX_TAGS, _DEV_MAX_TYPES = 256, 128           # limits of polus_bio_entity_counts


class EntityF1(IMetric):
    """Micro F1 over entities: both tag tensors of a batch are decoded by the BIO rule of polus_amd.ner.bio under one
    mask, and an entity counts as a true positive iff the other side has one with the same row, start, end and type.

    EntityF1(tags=[...names of the C tags in id order...]).  samples_from_batch takes (a, b) or (a, b, mask) of
    integer [B, S] (or [S]); mask nonzero = the token takes part (is_prediction, the attention mask, first wordpieces).
    The tuple order follows IConfusionMatrixTF._samples_from_batch, (y_true, y_pred): fp = entities of b alone,
    fn = entities of a alone.  F1 does not depend on the order; precision and recall are named by it, so under
    ValidationDataCallback, which keeps the reference's quirk of handing over (prediction, label), the two swap.

    Differences from the reference: no corpus object model, so entities are (row, start, end, type) over
    token columns and cannot continue from one row into the next; evaluate() returns 0.0 where the reference's
    precision_recall_f1 returns nan (nothing to count), as divide_no_nan does in the other metrics, so that
    SaveModelCallback(strategy="best") keeps working; tag ids outside [0, C) raise ValueError, at once on the host path
    and in evaluate() on the device path.

    evaluate() stores `last_results` before it resets: tp, fp, fn, precision, recall, f1, per_type (the same six per
    entity type), tags (the number of kept tokens) and the decode statistics under the reference's key names, each a
    pair (first tensor, second tensor)."""

    def __init__(self, *args, tags=None, reduce_f=None):
        if args or tags is None:
            raise TypeError("EntityF1(tags=[...tag names...]): the reference's EntityF1(corpora) decodes against the BioC "
                            "corpus object model (polus/ner/elements.py), which this port does not have; it works on tag "
                            "tensors, so pass the list of tag names as the keyword `tags`")
        super().__init__(reduce_f=reduce_f)
        self.tag_names = list(tags)
        self.scheme, self.type_names = bio.parse_scheme(self.tag_names)
        self.num_types = max(len(self.type_names), 1)
        self.last_results = None
        self._dev_scheme = {}
        self.reset()

    def reset(self):
        self._host_counts = np.zeros((self.num_types, 3), np.int64)
        self._host_stats = np.zeros(6, np.int64)
        self._dev_counts = self._dev_stats = None

    def _samples_from_batch(self, samples):
        if len(samples) == 3:
            a, b, mask = samples
        else:
            a, b = samples
            mask = None
        if (getattr(a, "is_cuda", False) and getattr(b, "is_cuda", False)
                and self.scheme.size <= _DEV_MAX_TAGS and self.num_types <= _DEV_MAX_TYPES):
            import torch
            from .. import ops
            dev = a.device
            if self._dev_counts is None:
                self._dev_counts = torch.zeros((self.num_types, 3), dtype=torch.int32, device=dev)
                self._dev_stats = torch.zeros(6, dtype=torch.int32, device=dev)
            if dev not in self._dev_scheme:
                self._dev_scheme[dev] = torch.as_tensor(self.scheme, device=dev)
            ta, m = bio.device_rows(a, mask)
            tb, _ = bio.device_rows(b, None)
            if ta.shape != tb.shape:
                raise ValueError(f"{self.name}: the two tag tensors differ in shape: {tuple(ta.shape)} and {tuple(tb.shape)}")
            ops.bio_entity_counts(ta, tb, self._dev_scheme[dev], self._dev_counts, self._dev_stats, mask=m)
            return
        # host arrays, and device tensors with more tags or types than the kernel keeps in LDS
        counts, stats = bio.entity_counts(a, b, self.scheme, mask=mask, num_types=self.num_types)
        if stats[1]:
            raise ValueError(self._rejected_message(int(stats[1])))
        self._host_counts += counts
        self._host_stats += stats

    def _rejected_message(self, bad):
        return f"{self.name}: {bad} tag value(s) outside [0, {self.scheme.size}) at positions that take part"

    def _evaluate(self):
        counts, stats = self._host_counts, self._host_stats
        if self._dev_counts is not None:           # the only device-to-host copies of the metric
            counts = counts + self._dev_counts.cpu().numpy()
            stats = stats + self._dev_stats.cpu().numpy()
        if stats[1]:
            raise ValueError(self._rejected_message(int(stats[1])))
        common, n_a, n_b = (counts[:, k].astype(np.float64) for k in range(3))
        tp, fn, fp = common, n_a - common, n_b - common
        f1 = lambda tp, fp, fn: _divide_no_nan(tp, tp + 0.5 * (fp + fn))  # noqa: E731
        per_type = {}
        for t, name in enumerate(self.type_names):
            per_type[name] = {"tp": int(tp[t]), "fp": int(fp[t]), "fn": int(fn[t]),
                              "precision": float(_divide_no_nan(tp[t], tp[t] + fp[t])),
                              "recall": float(_divide_no_nan(tp[t], tp[t] + fn[t])),
                              "f1": float(f1(tp[t], fp[t], fn[t]))}
        TP, FP, FN = tp.sum(), fp.sum(), fn.sum()
        self.last_results = {
            "tp": int(TP), "fp": int(FP), "fn": int(FN),
            "precision": float(_divide_no_nan(TP, TP + FP)), "recall": float(_divide_no_nan(TP, TP + FN)),
            "f1": float(f1(TP, FP, FN)), "per_type": per_type, "tags": int(stats[0]),
            "inside_tag_after_other_tag": (int(stats[2]), int(stats[4])),
            "inside_tag_with_different_entity_type": (int(stats[3]), int(stats[5])),
        }
        # the line of polus/ner/utils.py:127-130, once per side of the tuple
        for side, k in (("first", 2), ("second", 4)):
            logger.info("Statistics about the BIO decoding process ({} tensor): tags={}, inside_tag_after_other_tag={}, "
                        "inside_tag_with_different_entity_type={}.".format(side, int(stats[0]), int(stats[k]), int(stats[k + 1])))
        return self.last_results["f1"]
