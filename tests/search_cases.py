"""Cases, tolerances and stand-in models of the corpus search tests (tests/test_search_cpu.py, tests/test_search_gpu.py).

Tolerances of a search against float64 (absolute t = rel * max|score|):
  MaxSim  rel = maxsim_cases.TOL[mode]["score"], measured by the MaxSim kernel tests;
  dot     rel = 2e-5 * max(1, E / 64), the bound tests/test_kernels_gpu.py holds f32-output GEMMs to."""
import types

import numpy as np

from tests.maxsim_cases import TOL as MAXSIM_TOL

# N(0, 1) corpora searched against float64; k = 10 and 100
TOKEN_CASE = dict(seed=3, Q=16, N=3000, Lq=8, Ld=24, E=64, V=4096)
CLS_CASE = dict(seed=4, Q=16, N=5000, E=128)
KS = (10, 100)


def dot_tol(E):
    return 2e-5 * max(1.0, E / 64.0)


def maxsim_tol(mode):
    return MAXSIM_TOL[mode]["score"]


def token_case(seed, Q, N, Lq, Ld, E, V, integer=False):
    """A table of token vectors [V, E] and the token ids / masks of Q queries and N documents.  Ragged masks with
    holes; document 1 has no valid token; padding positions point at real (large) vectors."""
    r = np.random.Generator(np.random.PCG64(7000 + seed))
    table = r.integers(-2, 3, size=(V, E)).astype(np.float32) if integer else r.standard_normal((V, E)).astype(np.float32)
    q_ids, d_ids = r.integers(0, V, size=(Q, Lq)), r.integers(0, V, size=(N, Ld))
    ql, dl = r.integers(1, Lq + 1, size=Q), r.integers(1, Ld + 1, size=N)
    qm = (np.arange(Lq)[None] < ql[:, None]).astype(np.int32)
    dm = (np.arange(Ld)[None] < dl[:, None]).astype(np.int32)
    dm[r.random((N, Ld)) < 0.1] = 0
    dm[:, 0] = 1
    if N > 1:
        dm[1] = 0
    return dict(table=table, q_ids=q_ids.astype(np.int32), q_mask=qm, d_ids=d_ids.astype(np.int32), d_mask=dm)


def cls_case(seed, Q, N, E, integer=False):
    r = np.random.Generator(np.random.PCG64(8000 + seed))
    draw = (lambda s: r.integers(-3, 4, size=s).astype(np.float32)) if integer else (lambda s: r.standard_normal(s).astype(np.float32))
    table = draw((Q + N, E))
    return dict(table=table, q_ids=np.arange(Q, dtype=np.int32)[:, None], d_ids=(Q + np.arange(N, dtype=np.int32))[:, None],
                q_mask=np.ones((Q, 1), np.int32), d_mask=np.ones((N, 1), np.int32))


def batches(ids, mask, sizes, lengths=None):
    """The document dicts of several `add` calls: `sizes` documents each, cut to `lengths` tokens (None: all)."""
    out, a = [], 0
    for n, L in zip(sizes, lengths or [None] * len(sizes)):
        out.append({"input_ids": ids[a:a + n, :L], "attention_mask": mask[a:a + n, :L]})
        a += n
    assert a == len(ids)
    return out


class TableEncoder:
    """Stands in for a frozen BERT: the state of a token is its row of a table (device f32 [V, H])."""

    def __init__(self, table):
        import torch
        self.table = torch.as_tensor(table).cuda()
        self.config = types.SimpleNamespace(hidden_size=table.shape[1])

    def __call__(self, input_ids, attention_mask=None, training=False, **kw):
        import torch
        h = self.table[torch.as_tensor(np.asarray(input_ids)).long().cuda()]
        return types.SimpleNamespace(last_hidden_state=h, pooler_output=h[:, 0])


class TableModel:
    """A dual encoder whose projections are the identity: CorpusIndex sees exactly the table's rows, rounded to
    `dtype`, as [CLS] vectors (tokens=False: the first token's) or as token representations."""

    def __init__(self, table, dtype, tokens):
        self.enc, self.dtype, self.tokens = TableEncoder(table), dtype, tokens

    def _encode(self, x, training=False):
        import torch
        from polus_amd.ir.models import TokenReps
        out = self.enc(x["input_ids"])
        if not self.tokens:
            return out.pooler_output.to(self.dtype).contiguous()
        mask = torch.as_tensor(np.ascontiguousarray(x["attention_mask"])).to(torch.int32).cuda()
        return TokenReps(out.last_hidden_state.to(self.dtype).contiguous(), mask)

    encode_query = encode_document = _encode

    def query_projection(self, rep, training=False):
        return rep

    document_projection = query_projection
