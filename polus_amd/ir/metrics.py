"""Ranking metrics of a retrieval run through the IMetric protocol (polus_amd/metrics.py): Recall@k, MRR@k, nDCG@k.

A batch is `(ranked_ids, relevant)`: ranked_ids [Q, >= k] (a device tensor, as CorpusIndex.search returns it, or an
array; only the first k columns count and -1 is padding, no document), relevant one collection of document ids per
query (for NDCGAtK also one dict id -> gain per query).  The ids are a few kilobytes, so they come to the host and the
arithmetic is float64 NumPy; `evaluate()` is the mean over the queries seen since `reset()`."""
import numpy as np

from ..metrics import IMetric, _np


class _RankingMetric(IMetric):
    def __init__(self, k, reduce_f=None):
        super().__init__(reduce_f=reduce_f)
        if self.__class__.__name__ == "_RankingMetric":
            raise Exception("This is an interface that cannot be instantiated")
        if int(k) < 1:
            raise ValueError(f"k must be >= 1 (got {k})")
        self.k = int(k)
        self.name = f"{self._label}@{self.k}"
        self.reset()

    def reset(self):
        self._sum, self._n = 0.0, 0

    def _samples_from_batch(self, samples):
        ranked, relevant = samples
        ranked = _np(ranked)
        if ranked.ndim != 2 or ranked.shape[1] < self.k:
            raise ValueError(f"{self.name}: ranked ids must be [Q, >= {self.k}] (got shape {ranked.shape})")
        if len(relevant) != ranked.shape[0]:
            raise ValueError(f"{self.name}: {ranked.shape[0]} rankings but {len(relevant)} relevance collections")
        for row, rel in zip(ranked[:, :self.k].astype(np.int64), relevant):
            if len(rel) == 0:
                raise ValueError(f"{self.name}: a query without a relevant document has no defined value")
            self._sum += self._query(row, rel)
            self._n += 1

    def _evaluate(self):
        return float(self._sum / self._n) if self._n else 0.0


class RecallAtK(_RankingMetric):
    """|relevant in the top k| / |relevant|."""
    _label = "Recall"

    def _query(self, row, rel):
        rel = set(int(r) for r in rel)
        return len(rel.intersection(int(i) for i in row if i >= 0)) / float(len(rel))


class MRRAtK(_RankingMetric):
    """1 / rank of the first relevant document within the top k, else 0."""
    _label = "MRR"

    def _query(self, row, rel):
        rel = set(int(r) for r in rel)
        for rank, i in enumerate(row, 1):
            if i >= 0 and int(i) in rel:
                return 1.0 / rank
        return 0.0


class NDCGAtK(_RankingMetric):
    """Linear-gain nDCG (trec_eval ndcg_cut): DCG = sum over ranks i = 1..k of gain_i / log2(i + 1), over the DCG of
    the gains sorted descending.  `relevant` per query: a dict id -> gain, or a collection of ids (gain 1 each)."""
    _label = "nDCG"

    def _query(self, row, rel):
        gains = {int(i): float(g) for i, g in rel.items()} if isinstance(rel, dict) else {int(i): 1.0 for i in rel}
        disc = 1.0 / np.log2(np.arange(2, self.k + 2, dtype=np.float64))
        got = np.array([gains.get(int(i), 0.0) if i >= 0 else 0.0 for i in row], np.float64)
        ideal = np.sort(np.array(list(gains.values()), np.float64))[::-1][:self.k]
        idcg = float((ideal * disc[:len(ideal)]).sum())
        return float((got * disc).sum()) / idcg if idcg > 0 else 0.0
