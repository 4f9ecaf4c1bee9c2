"""The contract between a caller and the training-step and token-retrieval wrappers of polus_amd/ops.py, stated once.

The kernels take raw pointers, so a wrapper is the only place that can see a tensor's dtype, length and strides.  For every
wrapper of CORE_OPS and RETRIEVAL_OPS this table holds

  good()    the arguments of the smallest legal call, as CPU tensors (every optional tensor present), every extent exactly
            what the call touches (include/polus_hip.h): the rule a wrapper enforces is "at least this much", never "equal",
            because callers pass workspaces, padded arenas and `rows=` over a bigger tensor;
  entry     the entry points this call must reach, and expect() the pointer, stride and count arguments it must hand them;
  tensors   per tensor parameter, what is wrong with it in each family of mistakes (below); the bad calls are generated
            mechanically from good() by bad_cases();
  counts    count arguments (n_seg, rows=, cols=, C=) one larger than their tensors allow.

Families: "dtype" (f32 given as bf16, int32 as int64, the int64 tables as int32, tensors that must share a dtype given
different ones, an either-engine-dtype tensor given as float64), "extent" (one row, column or element fewer than the call
touches), "layout" (a non-unit inner stride where the entry point takes one row stride; a non-contiguous view where it takes a
flat pointer and a count), "count", "overlap" (two parameters the header calls distinct buffers given as overlapping views
of one allocation) and "device" (a host tensor).  A bad call must raise AssertionError or PolusHipError
before any entry point is reached, and the message must start with "<wrapper>: <parameter>" naming the mutated parameter or
one of the parameters its spec blames (the partner of a mismatch).  The device family keeps the shared `_req_cuda`, whose
message names neither.

Where the header makes a looser form legal the table says so instead of refusing it: embed_ln_fwd takes f32 tables with a
bf16 y (tables are f32 whatever the engine's dtype), and gemm / dense_thin take an f32 output or gradient beside bf16
operands.  Needs no GPU to import."""
import inspect

import numpy as np
import torch

from tests import fp8_ref, ivf_ref, maxsim_ref, residual_ref, search_ref, tuple_ref

F32, BF16, I32, I64, F64 = torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.float64
I16, U8, I8 = torch.int16, torch.uint8, torch.int8
SWAP = {F32: BF16, BF16: F32, I32: I64, I64: I32, I16: I32, U8: I8, I8: U8}
STREAM = 0xD00D                     # the dummy stream handle the recording library sees


class _Any:
    """Matches any recorded argument (workspace pointers and sizes)."""

    def __eq__(self, other):
        return True

    def __repr__(self):
        return "ANY"


ANY = _Any()

CORE_OPS = ("gemm", "dense_bwd_params", "dense_bwd_params_grouped", "dense_thin_fwd", "dense_thin_bwd", "attention_fwd",
            "attention_bwd", "layernorm_fwd", "layernorm_bwd", "layernorm_bwd_finalize", "embed_ln_fwd", "embed_ln_bwd",
            "colsum", "softmax_xent", "sigmoid_xent", "argmax", "confusion_matrix", "adam_step", "sqnorm", "sqnorm_segments",
            "clip_scale", "cast", "scale_", "act_bwd", "transpose_bf16", "transpose_bf16_batched", "dropout",
            "set_dynamic_params")

# the token-retrieval wrappers: MaxSim and normalisation, the FP8 and the residual index, top-k, centroids, inverted lists,
# tuples and distillation
RETRIEVAL_OPS = ("maxsim_fwd", "maxsim_bwd", "maxsim_scores", "maxsim_rerank", "l2norm_fwd", "l2norm_bwd",
                 "fp8_quantize", "fp8_dequantize", "maxsim_scores_fp8", "maxsim_rerank_fp8",
                 "residual_compress", "residual_decompress", "maxsim_rerank_res", "topk_merge",
                 "centroid_scores", "centroid_codes", "centroid_update", "centroid_scores_ids",
                 "ivf_count", "ivf_offsets", "ivf_fill", "ivf_mark", "ivf_compact",
                 "maxsim_tuples_fwd", "maxsim_tuples_bwd", "dot_tuples_fwd", "dot_tuples_bwd", "distill_kl", "margin_mse")

# every other public function of ops.py, none of them in this table: first the host-only route reports and the helpers, then
# the families left out so far
OTHER_OPS = ("workspace", "set_env", "reserve_cus", "gemm_route", "dense_bwd_params_route", "dense_bwd_params_grouped_route",
             "rowwise_route", "layernorm_bwd_partial_floats", "centroid_scores_route", "dense_thin_supported", "dropout_mask",
             # the wide masked-LM loss and the CRF wrappers
             "softmax_xent_wide_route", "softmax_xent_wide", "gather_rows", "inverse_map", "crf_nll", "crf_viterbi",
             # the sparse, lexical, postings, fusion, mining, pair and BIO wrappers: they name their parameters through _rows2d
             "splade_pool_fwd", "splade_pool_bwd", "flops_reg", "sparse_scores", "bm25_term_counts", "bm25_weights", "bm25_query",
             "postings_count", "postings_offsets", "postings_fill", "sparse_compact_rows", "bm25_query_lists",
             "postings_scores", "mine_negatives", "fuse_lists", "pair_lengths", "pair_pack",
             "pair_scatter_scores", "bio_entity_counts", "bio_spans")
# (the product-quantisation wrappers live in polus_amd/pq_ops.py and state their own contract there)


def public_functions(ops):
    return sorted(n for n, f in vars(ops).items()
                  if inspect.isfunction(f) and f.__module__ == ops.__name__ and not n.startswith("_"))


# ------------------------------------------------------------------------------------------------- the specification of a tensor
class T:
    """One tensor parameter.  bad: the wrong dtype to hand it.  ext: the shrinking views to try ("row": t[:-1], "col":
    t[:, :-1]).  layout: "inner" (one row stride is passed: a non-unit inner stride is wrong), "flat" (a flat pointer and a
    count: any non-contiguous view is wrong) or None (a single element).  blame: other parameters a refusal may name.
    out: written by the call (the GPU test carves it out of a guarded buffer)."""

    def __init__(self, bad, ext=("row",), layout="flat", blame=(), out=False):
        self.bad, self.ext, self.layout, self.blame, self.out = bad, tuple(ext), layout, tuple(blame), out


def fixed(dtype, **kw):
    """The header fixes the dtype."""
    return T(SWAP[dtype], **kw)


def same(**kw):
    """Shares the call's engine dtype (f32 in good()) with other parameters."""
    return T(BF16, **kw)


def free(**kw):
    """f32 or bf16, passed on as a dtype code of its own."""
    return T(F64, **kw)


class Case:
    def __init__(self, good, entry, tensors, scalars=(), counts=(), expect=None, overlaps=()):
        self.good, self.entry, self.tensors, self.scalars, self.counts, self.expect = good, tuple(entry), tensors, tuple(scalars), tuple(counts), expect
        self.overlaps = tuple(overlaps)         # (a, b): two parameters the header calls distinct buffers


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _f(a, dtype=F32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype)


def _nan(*shape, dtype=F32):
    return torch.full(shape, float("nan"), dtype=dtype)


def _neg(*shape, dtype=I32):
    return torch.full(shape, -1, dtype=dtype)


# ------------------------------------------------------------------------------------------------- good calls
GELU, ACT_FWD = 1, 2                # polus_hip.h: POLUS_ACT_GELU, POLUS_GEMM_ACT_FWD


def _gemm():
    r = _rng(1)
    return dict(a=_f(r.standard_normal((5, 8))), b=_f(r.standard_normal((6, 8))), out=_nan(5, 6), bias=_f(r.standard_normal(6)),
                resid=_f(r.standard_normal((5, 6))), aux=_nan(5, 6), act="gelu", flags=ACT_FWD)


def _dw():
    r = _rng(2)
    return dict(dy=_f(r.standard_normal((7, 6))), x=_f(r.standard_normal((7, 8))), dw=_nan(6, 8), db=_nan(6))


def _dw_grouped():
    r = _rng(3)
    return dict(problems=[(_f(r.standard_normal((7, 6))), _f(r.standard_normal((7, 8))), _nan(6, 8), _nan(6)),
                          (_f(r.standard_normal((7, 4))), _f(r.standard_normal((7, 8))), _nan(4, 8), _nan(4))])


def _thin_fwd():
    r = _rng(4)
    return dict(x=_f(r.standard_normal((5, 4))), w=_f(r.standard_normal((3, 4))), bias=_f(r.standard_normal(3)), y=_nan(5, 3))


def _thin_bwd():
    r = _rng(5)
    return dict(x=_f(r.standard_normal((5, 4))), dy=_f(r.standard_normal((5, 3))), w=_f(r.standard_normal((3, 4))), dx=_nan(5, 4),
                dw=_nan(3, 4), db=_nan(3))


ATT_B, ATT_S, ATT_A = 1, 17, 1


def _att_mask():
    m = torch.ones(ATT_B, ATT_S, dtype=I32)
    m[:, ATT_S - 3:] = 0
    return m


def _att_fwd():
    r = _rng(6)
    return dict(qkv=_f(r.standard_normal((ATT_B * ATT_S, 192))), mask=_att_mask(), ctx=_nan(ATT_B * ATT_S, 64),
                lse=_nan(ATT_B, ATT_A, ATT_S), B=ATT_B, S=ATT_S, n_heads=ATT_A)


def _att_bwd():
    r = _rng(6)
    qkv = _f(r.standard_normal((ATT_B * ATT_S, 192)))
    # ctx and lse are the forward's outputs; the GPU test fills them by running attention_fwd
    return dict(qkv=qkv, mask=_att_mask(), ctx=_f(r.standard_normal((ATT_B * ATT_S, 64))), dctx=_f(r.standard_normal((ATT_B * ATT_S, 64))),
                lse=_f(r.standard_normal((ATT_B, ATT_A, ATT_S))), dqkv=_nan(ATT_B * ATT_S, 192), B=ATT_B, S=ATT_S, n_heads=ATT_A)


LN_ROWS, LN_H, LN_EPS = 5, 4, 1e-12
LN_DROP_P, LN_SEED = 0.25, 11


def _ln_in(r):
    return _f(r.standard_normal((LN_ROWS, LN_H)) * 2 + 0.5), _f(1 + 0.1 * r.standard_normal(LN_H)), _f(0.1 * r.standard_normal(LN_H))


def _ln_fwd():
    x, g, b = _ln_in(_rng(7))
    return dict(x=x, gamma=g, beta=b, y=_nan(LN_ROWS, LN_H), mean=_nan(LN_ROWS), rstd=_nan(LN_ROWS), eps=LN_EPS)


def _ln_stats(x):
    x64 = x.double()
    mean = x64.mean(1)
    return mean.float(), (1.0 / torch.sqrt(x64.var(1, unbiased=False) + LN_EPS)).float()


def _ln_bwd():
    r = _rng(7)
    x, g, _ = _ln_in(r)
    mean, rstd = _ln_stats(x)
    return dict(dy=_f(r.standard_normal((LN_ROWS, LN_H))), x=x, gamma=g, mean=mean, rstd=rstd, dx=_nan(LN_ROWS, LN_H),
                dgamma=_nan(LN_H), dbeta=_nan(LN_H), dbias=_nan(LN_H), dx_masked=_nan(LN_ROWS, LN_H), drop_p=LN_DROP_P, seed=LN_SEED)


def _partial_floats():
    from polus_amd import ops
    return ops.layernorm_bwd_partial_floats(LN_ROWS, LN_H)


def _ln_bwd_deferred():
    p = _ln_bwd()
    p.update(dgamma=None, dbeta=None, partials=_nan(_partial_floats()))
    return p


def _ln_finalize():
    # the GPU test fills partials by running the deferred layernorm_bwd
    return dict(partials=torch.zeros(_partial_floats()), rows=LN_ROWS, H=LN_H, dgamma=_nan(LN_H), dbeta=_nan(LN_H), dbias=_nan(LN_H))


EMB_B, EMB_S, EMB_H, EMB_V, EMB_T = 2, 3, 4, 7, 2


def _emb_in():
    r = _rng(8)
    return dict(ids=_f(r.integers(0, EMB_V, size=(EMB_B, EMB_S)), I32), type_ids=_f(r.integers(0, EMB_T, size=(EMB_B, EMB_S)), I32),
                word=_f(r.standard_normal((EMB_V, EMB_H))), pos=_f(r.standard_normal((EMB_S, EMB_H))),
                typ=_f(r.standard_normal((EMB_T, EMB_H))), gamma=_f(1 + 0.1 * r.standard_normal(EMB_H))), r


def _emb_fwd():
    p, r = _emb_in()
    n = EMB_B * EMB_S
    p.update(beta=_f(0.1 * r.standard_normal(EMB_H)), y=_nan(n, EMB_H), mean=_nan(n), rstd=_nan(n), eps=LN_EPS)
    return p


def _emb_bwd():
    p, r = _emb_in()
    n = EMB_B * EMB_S
    pre = (p["word"][p["ids"].long()] + p["pos"][None, :EMB_S] + p["typ"][p["type_ids"].long()]).reshape(n, EMB_H)
    mean, rstd = _ln_stats(pre)
    r.standard_normal(EMB_H)        # beta's draw in _emb_fwd
    q = dict(dy=_f(r.standard_normal((n, EMB_H))))
    q.update(p)
    q.update(mean=mean, rstd=rstd, gword=_nan(EMB_V, EMB_H), gpos=_nan(EMB_S, EMB_H), gtyp=_nan(EMB_T, EMB_H), ggamma=_nan(EMB_H),
             gbeta=_nan(EMB_H))
    return q


def _colsum():
    return dict(x=_f(_rng(9).standard_normal((5, 6))), out=_nan(6))


def _softmax():
    r = _rng(10)
    return dict(logits=_f(r.standard_normal((4, 3)) * 3), labels=_f([0, 2, 1, 2], I32), loss=_nan(1), dlogits=_nan(4, 3),
                class_weights=_f(r.uniform(0.5, 2.0, size=3)))


def _sigmoid():
    r = _rng(11)
    return dict(logits=_f(r.standard_normal((4, 3)) * 3), y_true=_f(r.uniform(size=(4, 3)) < 0.4), class_weights=_f(r.uniform(0.5, 2.0, size=3)),
                negative_weight=0.5, loss=_nan(1), dlogits=_nan(4, 3))


def _argmax():
    return dict(x=_f(_rng(12).standard_normal((4, 3))), out=_neg(4))


def _confusion():
    return dict(row_idx=_f([0, 1, 2, 2, 5, 1], I32), col_idx=_f([0, 2, 2, 2, 1, -1], I32), cm=torch.zeros(3, 3, dtype=I32),
                rejected=torch.zeros(1, dtype=I32))


ADAM_SEG = ((0, 4, 1), (4, 7, 2))          # element 7 belongs to no window
# the first step of tests/rowwise_cases.py's optimizer (its ADAM_* constants, f32 values), so that its float64 reference applies
_f32 = lambda a: float(np.float32(a))
ADAM_HYPER = dict(lr=_f32(1e-2), lr_t=_f32(1e-2) * (1.0 - _f32(0.999)) ** 0.5 / (1.0 - _f32(0.9)), beta1=_f32(0.9), beta2=_f32(0.999),
                  eps=_f32(1e-7), weight_decay=_f32(0.01), grad_scale=1.0 / 64)
ADAM_CLIP = _f32(0.37)


def _adam():
    r = _rng(13)
    p = dict(p=_f(r.standard_normal(8)), g=_f(64 * r.standard_normal(8)), m=_f(0.1 * r.standard_normal(8)),
             v=_f(0.01 + 0.1 * r.uniform(size=8)), shadow=torch.zeros(8, dtype=BF16), seg=_f(ADAM_SEG, I64), n_seg=2)
    p.update(ADAM_HYPER)
    p["clip_scale"] = _f([ADAM_CLIP])
    return p


def _sqnorm():
    return dict(g=_f(_rng(14).standard_normal(9)), out=_nan(1))


def _sqnorm_seg():
    return dict(g=_f(_rng(15).standard_normal(8)), seg=_f(ADAM_SEG, I64), n_seg=2, out=_nan(1))


def _clip():
    return dict(sq=_f([3.0, 1.5]), grad_scale=0.5, clip_norm=0.7, out=_nan(1))


def _cast():
    return dict(src=_f(_rng(16).standard_normal(8)), dst=_nan(8, dtype=BF16))


def _scale():
    return dict(x=_f(_rng(17).standard_normal(8)), a=0.3)


def _act_bwd():
    r = _rng(18)
    return dict(dy=_f(r.standard_normal((2, 4))), u=_f(r.standard_normal((2, 4)) * 2), du=_nan(2, 4), act="gelu")


def _transpose():
    return dict(src=_f(_rng(19).standard_normal((3, 4)), BF16), dst=_nan(4, 3, dtype=BF16))


TR_SEGS = ((0, 3, 4, 0), (64, 4, 8, 1))    # (element offset, rows, cols, first tile): the 8-byte and the element path


def _transpose_batched():
    return dict(src_base=_f(_rng(20).standard_normal(96), BF16), dst_base=_nan(96, dtype=BF16), segs_dev=_f(TR_SEGS, I64), nseg=2,
                total_tiles=2)


def _dropout():
    return dict(x=_f(_rng(21).standard_normal((2, 4))), y=_nan(2, 4), drop_p=0.25, seed=7)


def _dyn_block():
    return dict(block=torch.zeros(4, dtype=I32))


# ------------------------------------------------------------------------------------------------- good calls: token retrieval
# B queries of Lq tokens, N documents of Ld tokens, E features, K centroids, C candidates per query, T rows, P probes per
# token: pairwise different, so that an argument in the wrong slot changes what the library is handed and what it computes
R_B, R_N, R_K, R_LD, R_LQ, R_C, R_T, R_P, R_E = 2, 3, 4, 5, 6, 7, 9, 8, 32
R_NBITS = 2
SLOT_MAJOR, QUERY_MAJOR = 0, 1      # polus_amd/ops.py


def _byte(*shape):
    return torch.full(shape, 0xAA, dtype=U8)


def _ms_in(seed, docs=R_N):
    """q [B, Lq, E], d [docs, Ld, E], masks with holes; masked positions hold large values, so counting one shows."""
    r = _rng(seed)
    q, d = r.standard_normal((R_B, R_LQ, R_E)), r.standard_normal((docs, R_LD, R_E))
    qm, dm = np.ones((R_B, R_LQ), np.int32), np.ones((docs, R_LD), np.int32)
    qm[0, 2], qm[1, 4:] = 0, 0
    dm[0, 1], dm[docs - 1, 3:], dm[1, 0] = 0, 0, 0
    q[qm == 0] *= 4.0
    d[dm == 0] *= 4.0
    return dict(q=_f(q), d=_f(d), qmask=_f(qm, I32), dmask=_f(dm, I32)), r


def _cand_ids():
    """int32 [B, C] names of documents, with one id on each side of [0, N)."""
    return _f([[2, 0, 1, -1, 1, 2, 0], [0, R_N, 2, 1, 0, 0, 2]], I32)


def _maxsim_fwd():
    p, _ = _ms_in(30)
    p.update(score=_nan(R_B, R_N), argmax=_neg(R_B, R_N, R_LQ))
    return p


def _maxsim_scores():
    p, _ = _ms_in(30)
    p.update(score=_nan(R_B, R_N))
    return p


def _maxsim_bwd():
    p, r = _ms_in(30)
    am = maxsim_ref.maxsim_fwd(p["q"].double().numpy(), p["d"].double().numpy(), p["qmask"].numpy(), p["dmask"].numpy())[1]
    return dict(q=p["q"], d=p["d"], dscore=_f(r.standard_normal((R_B, R_N))), argmax=_f(am, I32), dq=_nan(R_B, R_LQ, R_E),
                dd=_nan(R_N, R_LD, R_E))


def _maxsim_rerank():
    p, _ = _ms_in(30)
    p.update(cand=_cand_ids(), score=_nan(R_B, R_C))
    return p


def _l2_x():
    return _f(_rng(31).standard_normal((R_B, R_LQ, R_E)) * 3)


def _l2norm_fwd():
    return dict(x=_l2_x(), y=_nan(R_B, R_LQ, R_E), rnorm=_nan(R_B, R_LQ), eps=1e-12)


def _l2norm_bwd():
    # y and rnorm are the forward's outputs; the GPU test fills them by running l2norm_fwd
    y, rn = maxsim_ref.l2norm_fwd(_l2_x().double().numpy())
    return dict(y=_f(y), rnorm=_f(rn), dy=_f(_rng(32).standard_normal((R_B, R_LQ, R_E))), dx=_nan(R_B, R_LQ, R_E), eps=1e-12)


def _fp8_x():
    r = _rng(33)
    return _f(r.standard_normal((R_N, R_LD, R_E)) * np.exp2(r.integers(-6, 6, size=(R_N, R_LD, 1))))


def _fp8_quantize():
    return dict(x=_fp8_x(), codes=_byte(R_N, R_LD, R_E), scale=_nan(R_N, R_LD))


def _fp8_corpus():
    codes, scale, _ = fp8_ref.quantize(_fp8_x().numpy())
    return dict(codes=_f(codes, U8), scale=_f(scale))


def _fp8_dequantize():
    return dict(y=_nan(R_N, R_LD, R_E), **_fp8_corpus())


def _maxsim_scores_fp8():
    p, _ = _ms_in(30)
    p.pop("d")
    p.update(score=_nan(R_B, R_N), **_fp8_corpus())
    return p


def _maxsim_rerank_fp8():
    p = _maxsim_scores_fp8()
    p.update(cand=_cand_ids(), score=_nan(R_B, R_C))
    return p


def _tok_codes():
    """int16 [N, Ld] centroid codes (the bits of the unsigned code): 0xFFFF and 9 (>= K) are no token.  The lists:
    centroid 0 {0, 2}, 1 {0, 1}, 2 {1}, 3 {2}."""
    return _f(np.array([[0, 1, 1, 0xFFFF, 9], [1, 2, 0xFFFF, 2, 1], [3, 3, 0, 0xFFFF, 0xFFFF]], np.uint16).view(np.int16), I16)


def _res_codec():
    r = _rng(34)
    cent = r.standard_normal((R_K, R_E))
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    return dict(centroids=_f(cent), cutoffs=_f([-0.3, 0.05, 0.4]), weights=_f([-0.6, -0.1, 0.2, 0.7])), r


def _res_x(c, r):
    codes = residual_ref.codes_u16(_tok_codes().numpy())
    x = c["centroids"].numpy()[np.where(codes < R_K, codes, 0)] + 0.5 * r.standard_normal((R_N, R_LD, R_E)).astype(np.float32)
    return _f(x)


def _residual_compress():
    c, r = _res_codec()
    return dict(x=_res_x(c, r), codes=_tok_codes(), centroids=c["centroids"], cutoffs=c["cutoffs"], nbits=R_NBITS,
                packed=_byte(R_N, R_LD, R_E * R_NBITS // 8))


def _res_corpus():
    c, r = _res_codec()
    x, codes = _res_x(c, r), _tok_codes()
    packed = residual_ref.compress(x.numpy().reshape(-1, R_E), codes.numpy().reshape(-1), c["centroids"].numpy(), c["cutoffs"].numpy(), R_NBITS)
    return dict(codes=codes, packed=_f(packed.reshape(R_N, R_LD, -1), U8), centroids=c["centroids"], weights=c["weights"], nbits=R_NBITS)


def _residual_decompress():
    return dict(y=_nan(R_N, R_LD, R_E), **_res_corpus())


def _maxsim_rerank_res():
    p, _ = _ms_in(30)
    p.pop("d")
    p.update(cand=_cand_ids(), score=_nan(R_B, R_C), **_res_corpus())
    return p


def _topk_scores():
    s = _rng(35).standard_normal((R_B, R_C)).astype(np.float32)
    s[0, 1], s[0, 4], s[1, 2] = np.nan, -np.inf, s[1, 5]             # dropped, dropped, a tie (to the lower id)
    return s


TOPK_ID0 = 5


def _topk_merge():
    # the state of an earlier call over documents [0, TOPK_ID0), with one padding slot in row 1
    first = _rng(36).standard_normal((R_B, TOPK_ID0)).astype(np.float32)
    first[1, 1:3] = -np.inf
    val, idx = search_ref.topk(first, R_K)
    return dict(scores=_f(_topk_scores()), top_val=_f(val), top_id=_f(idx, I32), id0=TOPK_ID0, init=False)


def _topk_merge_ids():
    ids = np.array([[40, 3, 17, 9, 28, -1, 5], [6, 2, 31, 30, 8, 12, 1]], np.int32)
    return dict(scores=_f(_topk_scores()), top_val=_nan(R_B, R_K), top_id=torch.full((R_B, R_K), 12345, dtype=I32), init=True,
                ids=_f(ids, I32))


def _cs_in():
    qm = np.ones((R_B, R_LQ), np.int32)
    qm[0, 2], qm[1, 4:] = 0, 0
    return dict(table=_f(_rng(37).standard_normal((R_K, R_B * R_LQ))), qmask=_f(qm, I32), codes=_tok_codes())


def _centroid_scores():
    return dict(score=_nan(R_B, R_N), B=R_B, Lq=R_LQ, **_cs_in())


def _centroid_scores_ids():
    return dict(cand=_cand_ids(), score=_nan(R_B, R_C), B=R_B, Lq=R_LQ, **_cs_in())


def _centroid_codes():
    sim = _rng(38).standard_normal((R_T, R_K)).astype(np.float32)
    sim[2, 1], sim[4] = np.nan, np.nan                               # NaN never wins; a row of NaN codes 0
    mask = np.ones(R_T, np.int32)
    mask[5] = 0
    return dict(sim=_f(sim), mask=_f(mask, I32), codes=torch.full((R_T,), 1234, dtype=I16))


def _centroid_update():
    r = _rng(39)
    # centroid 2 has no row and keeps prev; 0xFFFF is no token
    codes = np.array([0, 1, 1, 3, 0xFFFF, 0, 3, 1, 0], np.uint16).view(np.int16)
    return dict(x=_f(r.standard_normal((R_T, R_E))), codes=_f(codes, I16), prev=_f(r.standard_normal((R_K, R_E))), out=_nan(R_K, R_E),
                counts=_neg(R_K), eps=1e-12)


def _ivf_lists():
    counts, offsets, members = ivf_ref.lists(residual_ref.codes_u16(_tok_codes().numpy()), R_K)
    return counts, offsets, np.concatenate(members)


def _ivf_count():
    return dict(codes=_tok_codes(), K=R_K, counts=_neg(R_K))


def _ivf_offsets():
    return dict(counts=_f(_ivf_lists()[0], I32), offsets=_neg(R_K + 1))


def _ivf_fill():
    _, offsets, docs = _ivf_lists()
    return dict(codes=_tok_codes(), offsets=_f(offsets, I32), cursor=_neg(R_K), docs=_neg(len(docs)))


def _ivf_mark():
    _, offsets, docs = _ivf_lists()
    probes = np.full((R_B, R_LQ, R_P), -1, np.int32)
    probes[0, 0, 3], probes[0, 2, 0] = 2, 0                          # query 0: centroid 2; token 2 is masked
    probes[1, 1, :2], probes[1, 5, 1] = (3, 7), 1                    # query 1: centroid 3 and an id past K; token 5 is masked
    qm = np.ones((R_B, R_LQ), np.int32)
    qm[0, 2], qm[1, 4:] = 0, 0
    return dict(probes=_f(probes.reshape(R_B * R_LQ, R_P), I32), qmask=_f(qm, I32), offsets=_f(offsets, I32), docs=_f(docs, I32), N=R_N,
                bitmap=_neg(R_B, 1), B=R_B, Lq=R_LQ)


def _ivf_compact():
    # row 0: more set bits than cap; row 1: one bit below N and one at N + 1, which does not count
    return dict(bitmap=_f([[0b111], [0b10010]], I32), N=R_N, count=_neg(R_B), cand=torch.full((R_B, 2), 77, dtype=I32))


def _tuples_fwd(layout):
    def good():
        p, _ = _ms_in(40, R_B * R_N)
        p.update(score=_nan(R_B, R_N), argmax=_neg(R_B, R_N, R_LQ), layout=layout)
        return p
    return good


def _tuples_bwd(layout):
    def good():
        p, r = _ms_in(40, R_B * R_N)
        am = tuple_ref.maxsim_tuples_fwd(p["q"].double().numpy(), p["d"].double().numpy(), p["qmask"].numpy(), p["dmask"].numpy(), layout)[1]
        return dict(q=p["q"], d=p["d"], dscore=_f(r.standard_normal((R_B, R_N))), argmax=_f(am, I32), dq=_nan(R_B, R_LQ, R_E),
                    dd=_nan(R_B * R_N, R_LD, R_E), layout=layout)
    return good


def _dot_in():
    r = _rng(41)
    return dict(q=_f(r.standard_normal((R_B, R_E))), d=_f(r.standard_normal((R_B * R_N, R_E)))), r


def _dot_fwd(layout):
    def good():
        p, _ = _dot_in()
        p.update(score=_nan(R_B, R_N), layout=layout)
        return p
    return good


def _dot_bwd(layout):
    def good():
        p, r = _dot_in()
        p.update(dscore=_f(r.standard_normal((R_B, R_N))), dq=_nan(R_B, R_E), dd=_nan(R_B * R_N, R_E), layout=layout)
        return p
    return good


def _distill():
    r = _rng(42)
    t = r.standard_normal((R_B, R_K)).astype(np.float32) * 2
    t[1, 2] = -np.inf                                                # an absent column
    return dict(student=_f(r.standard_normal((R_B, R_K)) * 2), teacher=_f(t), loss=_nan(1), dstudent=_nan(R_B, R_K))


# ------------------------------------------------------------------------------------------------- what the entry points must be handed
def _p(t):
    return None if t is None else t.data_ptr()


def _x_gemm(p):
    a, b, o = p["a"], p["b"], p["out"]
    return {"polus_gemm": (0, 0, 0, 0, _p(a), a.stride(0), _p(b), b.stride(0), _p(o), o.stride(0), 5, 6, 8, 1.0, _p(p["bias"]),
                           _p(p["resid"]), p["resid"].stride(0), _p(p["aux"]), p["aux"].stride(0), GELU, ACT_FWD, 1, None, 0, STREAM)}


def _x_dw(p):
    return {"polus_dense_bwd_params": (0, _p(p["dy"]), p["dy"].stride(0), _p(p["x"]), p["x"].stride(0), _p(p["dw"]), p["dw"].stride(0),
                                       _p(p["db"]), 7, 6, 8, 0, 1, ANY, ANY, STREAM)}


def _x_dw_grouped(p):
    return {"polus_dense_bwd_params_grouped": (0, 2, ANY, 7, 0, 1, ANY, ANY, STREAM)}


def _x_thin_fwd(p):
    x, w, y = p["x"], p["w"], p["y"]
    return {"polus_dense_thin_fwd": (0, _p(x), x.stride(0), _p(w), w.stride(0), _p(p["bias"]), 0, _p(y), y.stride(0), 5, 4, 3, STREAM)}


def _x_thin_bwd(p):
    x, dy, w, dx, dw = p["x"], p["dy"], p["w"], p["dx"], p["dw"]
    return {"polus_dense_thin_bwd": (0, _p(x), x.stride(0), 0, _p(dy), dy.stride(0), _p(w), w.stride(0), _p(dx), dx.stride(0),
                                     _p(dw), dw.stride(0), _p(p["db"]), 5, 4, 3, 0, ANY, ANY, STREAM)}


def _x_att_fwd(p):
    return {"polus_attention_fwd": (0, _p(p["qkv"]), _p(p["mask"]), _p(p["ctx"]), _p(p["lse"]), ATT_B, ATT_S, ATT_A, 64, 0.0, 0, STREAM)}


def _x_att_bwd(p):
    return {"polus_attention_bwd": (0, _p(p["qkv"]), _p(p["mask"]), _p(p["ctx"]), _p(p["dctx"]), _p(p["lse"]), _p(p["dqkv"]),
                                    ATT_B, ATT_S, ATT_A, 64, 0.0, 0, ANY, ANY, STREAM)}


def _x_ln_fwd(p):
    return {"polus_layernorm_fwd": (0, _p(p["x"]), _p(p["gamma"]), _p(p["beta"]), _p(p["y"]), _p(p["mean"]), _p(p["rstd"]),
                                    LN_ROWS, LN_H, LN_EPS, STREAM)}


def _x_ln_bwd(p):
    part = p.get("partials")
    return {"polus_layernorm_bwd": (0, _p(p["dy"]), _p(p["x"]), _p(p["gamma"]), _p(p["mean"]), _p(p["rstd"]), _p(p["dx"]),
                                    _p(p["dgamma"]), _p(p["dbeta"]), _p(p["dbias"]), 0, LN_ROWS, LN_H, _p(p["dx_masked"]), LN_DROP_P, LN_SEED,
                                    ANY if part is None else _p(part), ANY if part is None else part.numel() * 4, STREAM)}


def _x_ln_finalize(p):
    return {"polus_layernorm_bwd_finalize": (_p(p["partials"]), p["partials"].numel() * 4, LN_ROWS, LN_H, _p(p["dgamma"]), _p(p["dbeta"]),
                                             _p(p["dbias"]), 0, STREAM)}


def _x_emb_fwd(p):
    return {"polus_embed_ln_fwd": (0, _p(p["ids"]), _p(p["type_ids"]), _p(p["word"]), _p(p["pos"]), _p(p["typ"]), _p(p["gamma"]),
                                   _p(p["beta"]), _p(p["y"]), _p(p["mean"]), _p(p["rstd"]), EMB_B, EMB_S, EMB_H, EMB_V, EMB_S, EMB_T,
                                   LN_EPS, 0.0, 0, STREAM)}


def _x_emb_bwd(p):
    return {"polus_embed_ln_bwd": (0, _p(p["dy"]), _p(p["ids"]), _p(p["type_ids"]), _p(p["word"]), _p(p["pos"]), _p(p["typ"]),
                                   _p(p["gamma"]), _p(p["mean"]), _p(p["rstd"]), _p(p["gword"]), _p(p["gpos"]), _p(p["gtyp"]),
                                   _p(p["ggamma"]), _p(p["gbeta"]), 0, 0, EMB_B, EMB_S, EMB_H, EMB_V, EMB_S, EMB_T, 0.0, 0, ANY, ANY, STREAM)}


def _x_colsum(p):
    return {"polus_colsum": (0, _p(p["x"]), p["x"].stride(0), 5, 6, _p(p["out"]), 0, ANY, ANY, STREAM)}


def _x_softmax(p):
    return {"polus_softmax_xent": (0, _p(p["logits"]), p["logits"].stride(0), _p(p["labels"]), _p(p["class_weights"]), _p(p["loss"]),
                                   _p(p["dlogits"]), p["dlogits"].stride(0), 4, 3, ANY, ANY, STREAM)}


def _x_sigmoid(p):
    return {"polus_sigmoid_xent": (0, _p(p["logits"]), p["logits"].stride(0), _p(p["y_true"]), p["y_true"].stride(0), _p(p["class_weights"]),
                                   0.5, _p(p["loss"]), _p(p["dlogits"]), p["dlogits"].stride(0), 4, 3, ANY, ANY, STREAM)}


def _x_argmax(p):
    return {"polus_argmax": (_p(p["x"]), p["x"].stride(0), _p(p["out"]), 4, 3, STREAM)}


def _x_confusion(p):
    return {"polus_confusion_matrix": (_p(p["row_idx"]), _p(p["col_idx"]), 6, 3, _p(p["cm"]), _p(p["rejected"]), STREAM)}


def _x_adam(p):
    h = ADAM_HYPER
    return {"polus_adam_step": (_p(p["p"]), _p(p["g"]), _p(p["m"]), _p(p["v"]), _p(p["shadow"]), _p(p["seg"]), 2, 8, h["lr"], h["lr_t"],
                                h["beta1"], h["beta2"], h["eps"], h["weight_decay"], h["grad_scale"], _p(p["clip_scale"]), STREAM)}


def _x_sqnorm(p):
    return {"polus_sqnorm": (_p(p["g"]), 9, _p(p["out"]), ANY, ANY, STREAM)}


def _x_sqnorm_seg(p):
    return {"polus_sqnorm_segments": (_p(p["g"]), _p(p["seg"]), 2, _p(p["out"]), ANY, 4096, STREAM)}


def _x_clip(p):
    return {"polus_clip_scale": (_p(p["sq"]), 2, 0.5, 0.7, _p(p["out"]), STREAM)}


def _x_cast(p):
    return {"polus_cast": (0, _p(p["src"]), 1, _p(p["dst"]), 8, STREAM)}


def _x_scale(p):
    return {"polus_scale": (_p(p["x"]), 0.3, 8, STREAM)}


def _x_act_bwd(p):
    return {"polus_act_bwd": (0, _p(p["dy"]), _p(p["u"]), _p(p["du"]), 8, GELU, STREAM)}


def _x_transpose(p):
    return {"polus_transpose_bf16": (_p(p["src"]), _p(p["dst"]), 3, 4, STREAM)}


def _x_transpose_batched(p):
    return {"polus_transpose_bf16_batched": (_p(p["src_base"]), _p(p["dst_base"]), _p(p["segs_dev"]), 2, 2, STREAM)}


def _x_dropout(p):
    return {"polus_dropout": (0, _p(p["x"]), _p(p["y"]), 8, 0.25, 7, STREAM)}


def _x_dyn(p):
    return {"polus_set_dynamic_params": (_p(p["block"]),)}


def _ps(p, *names):
    return tuple(_p(p[n]) for n in names)


def _pld(t):
    return (_p(t), t.stride(0))


_MS_DIMS = (R_LQ, R_LD, R_E, STREAM)


def _x_maxsim_fwd(p):
    return {"polus_maxsim_fwd": (0,) + _ps(p, "q", "d", "qmask", "dmask") + _pld(p["score"]) + (_p(p["argmax"]), R_B, R_N) + _MS_DIMS}


def _x_maxsim_scores(p):
    return {"polus_maxsim_scores": (0,) + _ps(p, "q", "d", "qmask", "dmask") + _pld(p["score"]) + (R_B, R_N) + _MS_DIMS}


def _x_maxsim_bwd(p):
    return {"polus_maxsim_bwd": (0,) + _ps(p, "q", "d") + _pld(p["dscore"]) + _ps(p, "argmax", "dq", "dd") + (R_B, R_N) + _MS_DIMS}


def _x_maxsim_rerank(p):
    return {"polus_maxsim_rerank": (0,) + _ps(p, "q", "d", "qmask", "dmask") + _pld(p["cand"]) + _pld(p["score"]) + (R_B, R_C, R_N) + _MS_DIMS}


def _x_l2norm_fwd(p):
    return {"polus_l2norm_fwd": (0,) + _ps(p, "x", "y", "rnorm") + (R_B * R_LQ, R_E, 1e-12, STREAM)}


def _x_l2norm_bwd(p):
    return {"polus_l2norm_bwd": (0,) + _ps(p, "y", "rnorm", "dy", "dx") + (R_B * R_LQ, R_E, 1e-12, STREAM)}


def _x_fp8_quantize(p):
    return {"polus_fp8_quantize_rows": (0,) + _ps(p, "x", "codes", "scale") + (R_N * R_LD, R_E, STREAM)}


def _x_fp8_dequantize(p):
    return {"polus_fp8_dequantize_rows": (0,) + _ps(p, "codes", "scale", "y") + (R_N * R_LD, R_E, STREAM)}


def _x_maxsim_scores_fp8(p):
    return {"polus_maxsim_scores_fp8": (0,) + _ps(p, "q", "codes", "scale", "qmask", "dmask") + _pld(p["score"]) + (R_B, R_N) + _MS_DIMS}


def _x_maxsim_rerank_fp8(p):
    return {"polus_maxsim_rerank_fp8": (0,) + _ps(p, "q", "codes", "scale", "qmask", "dmask") + _pld(p["cand"]) + _pld(p["score"])
            + (R_B, R_C, R_N) + _MS_DIMS}


def _x_residual_compress(p):
    return {"polus_residual_compress": (0,) + _ps(p, "x", "codes", "centroids") + (R_K, _p(p["cutoffs"]), R_NBITS, _p(p["packed"]),
                                                                                 R_N * R_LD, R_E, STREAM)}


def _x_residual_decompress(p):
    return {"polus_residual_decompress": (0,) + _ps(p, "codes", "packed", "centroids") + (R_K, _p(p["weights"]), R_NBITS, _p(p["y"]),
                                                                                       R_N * R_LD, R_E, STREAM)}


def _x_maxsim_rerank_res(p):
    return {"polus_maxsim_rerank_res": (0,) + _ps(p, "q", "codes", "packed", "centroids") + (R_K, _p(p["weights"]), R_NBITS)
            + _ps(p, "qmask", "dmask") + _pld(p["cand"]) + _pld(p["score"]) + (R_B, R_C, R_N) + _MS_DIMS}


def _x_topk_merge(p):
    return {"polus_topk_merge": _pld(p["scores"]) + (R_B, R_C, TOPK_ID0) + _ps(p, "top_val", "top_id") + (R_K, 0, STREAM)}


def _x_topk_merge_ids(p):
    return {"polus_topk_merge_ids": _pld(p["scores"]) + _pld(p["ids"]) + (R_B, R_C) + _ps(p, "top_val", "top_id") + (R_K, 1, STREAM)}


def _x_centroid_scores(p):
    return {"polus_centroid_scores": _pld(p["table"]) + _ps(p, "qmask", "codes") + _pld(p["score"]) + (R_B, R_N, R_LQ, R_LD, R_K, STREAM)}


def _x_centroid_scores_ids(p):
    return {"polus_centroid_scores_ids": _pld(p["table"]) + _ps(p, "qmask", "codes") + _pld(p["cand"]) + _pld(p["score"])
            + (R_B, R_C, R_N, R_LQ, R_LD, R_K, STREAM)}


def _x_centroid_codes(p):
    return {"polus_centroid_codes": _pld(p["sim"]) + _ps(p, "mask", "codes") + (R_T, R_K, STREAM)}


def _x_centroid_update(p):
    return {"polus_centroid_update": (0,) + _ps(p, "x", "codes", "prev", "out", "counts") + (R_T, R_K, R_E, 1e-12, STREAM)}


IVF_PAIRS = 6                       # the (centroid, document) pairs of _tok_codes()


def _x_ivf_count(p):
    return {"polus_ivf_count": (_p(p["codes"]), R_N, R_LD, R_K, _p(p["counts"]), STREAM)}


def _x_ivf_offsets(p):
    return {"polus_ivf_offsets": (_p(p["counts"]), R_K, _p(p["offsets"]), STREAM)}


def _x_ivf_fill(p):
    return {"polus_ivf_fill": (_p(p["codes"]), R_N, R_LD, R_K, _p(p["offsets"]), IVF_PAIRS, _p(p["cursor"]), _p(p["docs"]), STREAM)}


def _x_ivf_mark(p):
    return {"polus_ivf_mark": _pld(p["probes"]) + _ps(p, "qmask", "offsets", "docs") + (IVF_PAIRS, R_K, R_N) + _pld(p["bitmap"])
            + (R_B, R_LQ, R_P, STREAM)}


def _x_ivf_compact(p):
    return {"polus_ivf_compact": _pld(p["bitmap"]) + (R_B, R_N) + _pld(p["cand"]) + (2, _p(p["count"]), STREAM)}


def _x_tuples_fwd(p):
    return {"polus_maxsim_tuples_fwd": (0,) + _ps(p, "q", "d", "qmask", "dmask") + _pld(p["score"]) + (_p(p["argmax"]), R_B, R_N, p["layout"])
            + _MS_DIMS}


def _x_tuples_bwd(p):
    return {"polus_maxsim_tuples_bwd": (0,) + _ps(p, "q", "d") + _pld(p["dscore"]) + _ps(p, "argmax", "dq", "dd") + (R_B, R_N, p["layout"])
            + _MS_DIMS}


def _x_dot_fwd(p):
    return {"polus_dot_tuples_fwd": (0,) + _pld(p["q"]) + _pld(p["d"]) + _pld(p["score"]) + (R_B, R_N, p["layout"], R_E, STREAM)}


def _x_dot_bwd(p):
    return {"polus_dot_tuples_bwd": (0,) + _pld(p["q"]) + _pld(p["d"]) + _pld(p["dscore"]) + _pld(p["dq"]) + _pld(p["dd"])
            + (R_B, R_N, p["layout"], R_E, STREAM)}


def _x_distill(fn):
    def expect(p):
        return {fn: _pld(p["student"]) + _pld(p["teacher"]) + (_p(p["loss"]),) + _pld(p["dstudent"]) + (R_B, R_K, ANY, ANY, STREAM)}
    return expect


# ------------------------------------------------------------------------------------------------- the table
_vec32 = lambda **kw: fixed(F32, **kw)
_one = lambda dtype=F32, **kw: fixed(dtype, layout=None, **kw)          # a single element: no layout to get wrong
_mat = dict(ext=("row", "col"), layout="inner")

_EMB_SHARED = dict(ids=fixed(I32, ext=()), type_ids=fixed(I32),
                   word=fixed(F32, ext=(), blame=("pos", "typ", "gamma")), pos=fixed(F32), typ=fixed(F32, ext=()), gamma=_vec32(),
                   mean=_vec32(out=False), rstd=_vec32(out=False))
_LN_BWD = dict(dy=same(blame=("x",)), x=same(blame=("dy", "dx")), gamma=_vec32(), mean=_vec32(), rstd=_vec32(), dx=same(out=True),
               dbias=_vec32(out=True), dx_masked=same(out=True))
_LN_BWD_SCALARS = ("accumulate", "drop_p", "seed")
_ATT = dict(qkv=same(blame=("ctx", "dqkv", "dctx")), mask=fixed(I32), lse=fixed(F32))

CASES = {
    "gemm": Case(_gemm, ["polus_gemm"], dict(a=same(blame=("b",), ext=("col",), layout="inner"), b=same(ext=("col",), layout="inner"), out=same(out=True, **_mat),
                                             bias=_vec32(), resid=same(**_mat), aux=same(out=True, **_mat)),
                 scalars=("a_layout", "b_layout", "M", "N", "K", "alpha", "act", "flags", "split_k", "drop_p", "seed"),
                 counts=(("M", 6, ("a", "out")), ("N", 7, ("b", "out")), ("K", 9, ("a",))), expect=_x_gemm),
    "dense_bwd_params": Case(_dw, ["polus_dense_bwd_params"],
                             dict(dy=same(blame=("x", "dw"), **_mat), x=same(blame=("dw",), **_mat), dw=fixed(F32, out=True, **_mat),
                                  db=_vec32(out=True)), scalars=("accumulate", "split_k"), expect=_x_dw),
    "dense_bwd_params_grouped": Case(_dw_grouped, ["polus_dense_bwd_params_grouped"],
                                     {"problems[0].dy": same(**_mat), "problems[1].x": same(**_mat),
                                      "problems[1].dw": fixed(F32, out=True, **_mat), "problems[0].dw": fixed(F32, out=True, ext=(), layout=None),
                                      "problems[0].db": _vec32(out=True), "problems[1].db": _vec32(out=True)},
                                     scalars=("accumulate", "split_k"), expect=_x_dw_grouped),
    "dense_thin_fwd": Case(_thin_fwd, ["polus_dense_thin_fwd"], dict(x=same(blame=("w", "y"), **_mat), w=same(blame=("y",), **_mat),
                                                                     bias=_vec32(), y=same(out=True, **_mat)), expect=_x_thin_fwd),
    "dense_thin_bwd": Case(_thin_bwd, ["polus_dense_thin_bwd"],
                           dict(x=same(blame=("w", "dy", "dx"), **_mat), dy=same(**_mat), w=same(blame=("dy", "dw"), **_mat),
                                dx=same(out=True, **_mat), dw=fixed(F32, out=True, **_mat), db=_vec32(out=True)),
                           scalars=("accumulate",), expect=_x_thin_bwd),
    "attention_fwd": Case(_att_fwd, ["polus_attention_fwd"], {**_ATT, "ctx": same(out=True), "lse": fixed(F32, out=True)},
                          scalars=("B", "S", "n_heads", "drop_p", "seed"), expect=_x_att_fwd),
    "attention_bwd": Case(_att_bwd, ["polus_attention_bwd"], dict(ctx=same(), dctx=same(), dqkv=same(out=True), **_ATT),
                          scalars=("B", "S", "n_heads", "drop_p", "seed"), expect=_x_att_bwd),
    "layernorm_fwd": Case(_ln_fwd, ["polus_layernorm_fwd"], dict(x=same(blame=("y",)), gamma=_vec32(), beta=_vec32(), y=same(out=True),
                                                                 mean=_vec32(out=True), rstd=_vec32(out=True)),
                          scalars=("eps",), expect=_x_ln_fwd),
    "layernorm_bwd": Case(_ln_bwd, ["polus_layernorm_bwd"], dict(dgamma=_vec32(out=True), dbeta=_vec32(out=True), **_LN_BWD),
                          scalars=_LN_BWD_SCALARS + ("partials",), expect=_x_ln_bwd),
    "layernorm_bwd:deferred": Case(_ln_bwd_deferred, ["polus_layernorm_bwd"], dict(partials=_vec32(out=True), **_LN_BWD),
                                   scalars=_LN_BWD_SCALARS + ("dgamma", "dbeta"), expect=_x_ln_bwd),
    "layernorm_bwd_finalize": Case(_ln_finalize, ["polus_layernorm_bwd_finalize"],
                                   dict(partials=_vec32(), dgamma=_vec32(out=True), dbeta=_vec32(out=True), dbias=_vec32(out=True)),
                                   scalars=("rows", "H", "accumulate"), counts=(("rows", 100000, ("partials",)), ("H", 8, ("partials", "dgamma"))),
                                   expect=_x_ln_finalize),
    "embed_ln_fwd": Case(_emb_fwd, ["polus_embed_ln_fwd"], {**_EMB_SHARED, "beta": _vec32(), "y": free(out=True),
                                                                "mean": _vec32(out=True), "rstd": _vec32(out=True)},
                         scalars=("eps", "drop_p", "seed"), expect=_x_emb_fwd),
    "embed_ln_bwd": Case(_emb_bwd, ["polus_embed_ln_bwd"], dict(dy=free(), gword=_vec32(out=True), gpos=_vec32(out=True), gtyp=_vec32(out=True),
                                                                ggamma=_vec32(out=True), gbeta=_vec32(out=True), **_EMB_SHARED),
                         scalars=("accumulate", "deterministic", "drop_p", "seed"), expect=_x_emb_bwd),
    "colsum": Case(_colsum, ["polus_colsum"], dict(x=free(ext=(), layout="inner"), out=_vec32(out=True)), scalars=("accumulate",),
                   counts=(("rows", 6, ("x",)), ("cols", 7, ("x", "out"))), expect=_x_colsum),
    "softmax_xent": Case(_softmax, ["polus_softmax_xent"], dict(logits=fixed(F32, ext=(), layout="inner", blame=("labels", "dlogits", "class_weights")),
                                                                labels=fixed(I32), loss=_one(out=True), dlogits=free(out=True, **_mat),
                                                                class_weights=_vec32()),
                         counts=(("rows", 5, ("logits", "labels", "dlogits")), ("C", 4, ("logits", "dlogits", "class_weights"))), expect=_x_softmax),
    "sigmoid_xent": Case(_sigmoid, ["polus_sigmoid_xent"], dict(logits=fixed(F32, ext=(), layout="inner", blame=("y_true", "dlogits", "class_weights")),
                                                                y_true=fixed(F32, **_mat), class_weights=_vec32(), loss=_one(out=True),
                                                                dlogits=free(out=True, **_mat)),
                         scalars=("negative_weight",), expect=_x_sigmoid),
    "argmax": Case(_argmax, ["polus_argmax"], dict(x=fixed(F32, ext=(), layout="inner", blame=("out",)), out=fixed(I32, out=True)),
                   counts=(("rows", 5, ("x", "out")), ("C", 4, ("x",))), expect=_x_argmax),
    "confusion_matrix": Case(_confusion, ["polus_confusion_matrix"], dict(row_idx=fixed(I32, blame=("col_idx",)), col_idx=fixed(I32),
                                                                         cm=fixed(I32, out=True), rejected=_one(I32, out=True)), expect=_x_confusion),
    "adam_step": Case(_adam, ["polus_adam_step"], dict(p=_vec32(out=True, ext=()), g=_vec32(), m=_vec32(out=True), v=_vec32(out=True),
                                                       shadow=fixed(BF16, out=True), seg=fixed(I64), clip_scale=_one()),
                      scalars=("n_seg", "lr", "lr_t", "beta1", "beta2", "eps", "weight_decay", "grad_scale"), counts=(("n_seg", 3, ("seg",)),),
                      expect=_x_adam),
    "sqnorm": Case(_sqnorm, ["polus_sqnorm"], dict(g=_vec32(ext=()), out=_one(out=True)), expect=_x_sqnorm),
    "sqnorm_segments": Case(_sqnorm_seg, ["polus_sqnorm_segments"], dict(g=_vec32(ext=()), seg=fixed(I64), out=_one(out=True)),
                            scalars=("n_seg",), counts=(("n_seg", 3, ("seg",)),), expect=_x_sqnorm_seg),
    "clip_scale": Case(_clip, ["polus_clip_scale"], dict(sq=_vec32(ext=()), out=_one(out=True)), scalars=("grad_scale", "clip_norm"), expect=_x_clip),
    "cast": Case(_cast, ["polus_cast"], dict(src=free(blame=("dst",)), dst=free(out=True)), expect=_x_cast),
    "scale_": Case(_scale, ["polus_scale"], dict(x=_vec32(out=True, ext=())), scalars=("a",), expect=_x_scale),
    "act_bwd": Case(_act_bwd, ["polus_act_bwd"], dict(dy=same(blame=("u", "du")), u=same(), du=same(out=True)), scalars=("act",), expect=_x_act_bwd),
    "transpose_bf16": Case(_transpose, ["polus_transpose_bf16"], dict(src=fixed(BF16, blame=("dst",)), dst=fixed(BF16, out=True)), expect=_x_transpose),
    "transpose_bf16_batched": Case(_transpose_batched, ["polus_transpose_bf16_batched"],
                                   dict(src_base=fixed(BF16, ext=()), dst_base=fixed(BF16, out=True), segs_dev=fixed(I64)),
                                   scalars=("nseg", "total_tiles"), counts=(("nseg", 3, ("segs_dev",)),), expect=_x_transpose_batched),
    "dropout": Case(_dropout, ["polus_dropout"], dict(x=same(blame=("y",)), y=same(out=True)), scalars=("drop_p", "seed"), expect=_x_dropout),
    "set_dynamic_params": Case(_dyn_block, ["polus_set_dynamic_params"], dict(block=T(None)), expect=_x_dyn),
}

# ---- token retrieval
_mask = lambda **kw: fixed(I32, **kw)
_score = lambda **kw: fixed(F32, out=True, ext=("row", "col"), layout="inner", **kw)
_cand = lambda **kw: fixed(I32, ext=("row", "col"), layout="inner", blame=("score",), **kw)
_codes2 = lambda **kw: fixed(I16, ext=(), **kw)                       # [N, Ld]: defines N and Ld (EXEMPT)
_RERANK = dict(qmask=_mask(), dmask=_mask(), cand=_cand(), score=_score())
_CS = dict(table=fixed(F32, ext=("col",), layout="inner"), qmask=_mask(), codes=_codes2())
_CS_COUNTS = (("B", R_B + 1, ("table", "qmask", "score")), ("Lq", R_LQ + 1, ("table", "qmask")))
_RES = dict(codes=fixed(I16), centroids=same(ext=("col",)))
_TUPLE_KEYS = (("", SLOT_MAJOR), (":query_major", QUERY_MAJOR))

CASES.update({
    "maxsim_fwd": Case(_maxsim_fwd, ["polus_maxsim_fwd"],
                       dict(q=same(blame=("d", "qmask", "argmax")), d=same(blame=("dmask", "argmax")), qmask=_mask(), dmask=_mask(),
                            score=_score(), argmax=fixed(I32, out=True)), expect=_x_maxsim_fwd),
    "maxsim_scores": Case(_maxsim_scores, ["polus_maxsim_scores"],
                          dict(q=same(blame=("d", "qmask")), d=same(blame=("dmask",)), qmask=_mask(), dmask=_mask(), score=_score()),
                          expect=_x_maxsim_scores),
    "maxsim_bwd": Case(_maxsim_bwd, ["polus_maxsim_bwd"],
                       dict(q=same(blame=("d", "argmax")), d=same(blame=("argmax",)), dscore=fixed(F32, **_mat), argmax=fixed(I32),
                            dq=same(out=True), dd=same(out=True)), expect=_x_maxsim_bwd),
    "maxsim_rerank": Case(_maxsim_rerank, ["polus_maxsim_rerank"], dict(q=same(blame=("d", "cand")), d=same(blame=("dmask",)), **_RERANK),
                          expect=_x_maxsim_rerank),
    "l2norm_fwd": Case(_l2norm_fwd, ["polus_l2norm_fwd"], dict(x=same(blame=("y", "rnorm")), y=same(out=True), rnorm=fixed(F32, out=True)),
                       scalars=("eps",), expect=_x_l2norm_fwd),
    "l2norm_bwd": Case(_l2norm_bwd, ["polus_l2norm_bwd"], dict(y=same(blame=("rnorm", "dy")), rnorm=fixed(F32), dy=same(), dx=same(out=True)),
                       scalars=("eps",), expect=_x_l2norm_bwd),
    "fp8_quantize": Case(_fp8_quantize, ["polus_fp8_quantize_rows"],
                         dict(x=free(blame=("codes",)), codes=fixed(U8, out=True), scale=fixed(F32, out=True)), expect=_x_fp8_quantize),
    "fp8_dequantize": Case(_fp8_dequantize, ["polus_fp8_dequantize_rows"],
                           dict(codes=fixed(U8), scale=fixed(F32), y=free(out=True, blame=("codes",))), expect=_x_fp8_dequantize),
    "maxsim_scores_fp8": Case(_maxsim_scores_fp8, ["polus_maxsim_scores_fp8"],
                              dict(q=free(blame=("qmask",)), codes=fixed(U8, blame=("scale",)), scale=fixed(F32), qmask=_mask(), dmask=_mask(),
                                   score=_score()), expect=_x_maxsim_scores_fp8),
    "maxsim_rerank_fp8": Case(_maxsim_rerank_fp8, ["polus_maxsim_rerank_fp8"],
                              dict(q=free(blame=("cand",)), codes=fixed(U8, blame=("scale",)), scale=fixed(F32), **_RERANK),
                              expect=_x_maxsim_rerank_fp8),
    "residual_compress": Case(_residual_compress, ["polus_residual_compress"],
                              dict(x=same(blame=("codes", "centroids")), cutoffs=fixed(F32), packed=fixed(U8, out=True), **_RES),
                              scalars=("nbits",), expect=_x_residual_compress),
    "residual_decompress": Case(_residual_decompress, ["polus_residual_decompress"],
                                dict(packed=fixed(U8), weights=fixed(F32), y=same(out=True, blame=("codes", "centroids")), **_RES),
                                scalars=("nbits",), expect=_x_residual_decompress),
    "maxsim_rerank_res": Case(_maxsim_rerank_res, ["polus_maxsim_rerank_res"],
                              dict(q=same(blame=("centroids", "cand")), codes=fixed(I16, blame=("packed",)), packed=fixed(U8),
                                   centroids=same(ext=("col",)), weights=fixed(F32), **_RERANK),
                              scalars=("nbits",), expect=_x_maxsim_rerank_res),
    "topk_merge": Case(_topk_merge, ["polus_topk_merge"],
                       dict(scores=fixed(F32, layout="inner", blame=("top_val",)), top_val=fixed(F32, out=True, ext=("row", "col"), blame=("top_id",)),
                            top_id=fixed(I32, out=True, ext=("row", "col"))), scalars=("id0", "init", "ids"), expect=_x_topk_merge),
    "topk_merge:ids": Case(_topk_merge_ids, ["polus_topk_merge_ids"],
                           dict(scores=fixed(F32, layout="inner", blame=("top_val",)), top_val=fixed(F32, out=True, ext=("row", "col"), blame=("top_id",)),
                                top_id=fixed(I32, out=True, ext=("row", "col")), ids=fixed(I32, ext=("row", "col"), layout="inner")),
                           scalars=("id0", "init"), expect=_x_topk_merge_ids),
    "centroid_scores": Case(_centroid_scores, ["polus_centroid_scores"], dict(score=_score(), **_CS), counts=_CS_COUNTS, expect=_x_centroid_scores),
    "centroid_scores_ids": Case(_centroid_scores_ids, ["polus_centroid_scores_ids"],
                                dict(cand=fixed(I32, layout="inner"), score=_score(), **_CS), counts=_CS_COUNTS, expect=_x_centroid_scores_ids),
    "centroid_codes": Case(_centroid_codes, ["polus_centroid_codes"], dict(sim=fixed(F32, ext=(), layout="inner"), mask=_mask(), codes=fixed(I16, out=True)),
                           counts=(("rows", R_T + 1, ("sim", "mask", "codes")), ("K", R_K + 1, ("sim",))), expect=_x_centroid_codes),
    "centroid_update": Case(_centroid_update, ["polus_centroid_update"],
                            dict(x=same(blame=("prev", "codes")), codes=fixed(I16), prev=same(blame=("out",)), out=same(out=True),
                                 counts=fixed(I32, out=True)), scalars=("eps",), overlaps=(("out", "prev"),), expect=_x_centroid_update),
    "ivf_count": Case(_ivf_count, ["polus_ivf_count"], dict(codes=_codes2(), counts=fixed(I32, out=True)), counts=(("K", R_K + 1, ("counts",)),),
                      expect=_x_ivf_count),
    "ivf_offsets": Case(_ivf_offsets, ["polus_ivf_offsets"], dict(counts=fixed(I32, blame=("offsets",)), offsets=fixed(I32, out=True)),
                        expect=_x_ivf_offsets),
    "ivf_fill": Case(_ivf_fill, ["polus_ivf_fill"], dict(codes=_codes2(), offsets=fixed(I32), cursor=fixed(I32, out=True, blame=("offsets",)),
                                                         docs=fixed(I32, out=True, ext=())), expect=_x_ivf_fill),
    "ivf_mark": Case(_ivf_mark, ["polus_ivf_mark"], dict(probes=fixed(I32, layout="inner"), qmask=_mask(), offsets=fixed(I32, ext=()),
                                                         docs=fixed(I32, ext=()), bitmap=fixed(I32, out=True, **_mat)),
                     counts=(("N", 33, ("bitmap",)), ("B", R_B + 1, ("probes", "qmask", "bitmap")), ("Lq", R_LQ + 1, ("probes", "qmask"))),
                     expect=_x_ivf_mark),
    "ivf_compact": Case(_ivf_compact, ["polus_ivf_compact"], dict(bitmap=fixed(I32, **_mat), count=fixed(I32, out=True, ext=()),
                                                                  cand=fixed(I32, out=True, layout="inner")),
                        counts=(("N", 33, ("bitmap",)),), expect=_x_ivf_compact),
    "distill_kl": Case(_distill, ["polus_distill_kl"], dict(student=fixed(F32, blame=("teacher",), **_mat), teacher=fixed(F32, **_mat),
                                                            loss=_one(out=True), dstudent=fixed(F32, out=True, **_mat)),
                       expect=_x_distill("polus_distill_kl")),
    "margin_mse": Case(_distill, ["polus_margin_mse"], dict(student=fixed(F32, blame=("teacher",), **_mat), teacher=fixed(F32, **_mat),
                                                            loss=_one(out=True), dstudent=fixed(F32, out=True, **_mat)),
                       expect=_x_distill("polus_margin_mse")),
})
for _suffix, _layout in _TUPLE_KEYS:
    CASES.update({
        "maxsim_tuples_fwd" + _suffix: Case(_tuples_fwd(_layout), ["polus_maxsim_tuples_fwd"],
                                            dict(q=same(blame=("d", "score", "argmax")), d=same(blame=("dmask", "argmax")), qmask=_mask(),
                                                 dmask=_mask(), score=_score(), argmax=fixed(I32, out=True)),
                                            scalars=("layout",), expect=_x_tuples_fwd),
        "maxsim_tuples_bwd" + _suffix: Case(_tuples_bwd(_layout), ["polus_maxsim_tuples_bwd"],
                                            dict(q=same(blame=("d", "dscore", "argmax")), d=same(blame=("argmax",)), dscore=fixed(F32, **_mat),
                                                 argmax=fixed(I32), dq=same(out=True), dd=same(out=True)),
                                            scalars=("layout",), expect=_x_tuples_bwd),
        "dot_tuples_fwd" + _suffix: Case(_dot_fwd(_layout), ["polus_dot_tuples_fwd"],
                                         dict(q=same(blame=("d", "score"), **_mat), d=same(**_mat), score=_score()),
                                         scalars=("layout",), expect=_x_dot_fwd),
        "dot_tuples_bwd" + _suffix: Case(_dot_bwd(_layout), ["polus_dot_tuples_bwd"],
                                         dict(q=same(blame=("d", "dscore", "dq"), **_mat), d=same(blame=("dd",), **_mat), dscore=fixed(F32, **_mat),
                                              dq=same(out=True, **_mat), dd=same(out=True, **_mat)),
                                         scalars=("layout",), expect=_x_dot_bwd),
    })

# (wrapper, parameter, family) -> why no bad case of that family exists
EXEMPT = {
    ("embed_ln_fwd", "word", "extent"): "word defines V and H; fewer rows are a smaller vocabulary, which the kernel clamps ids against",
    ("embed_ln_bwd", "word", "extent"): "as embed_ln_fwd: word defines V, and gword is then checked against that V",
    ("embed_ln_fwd", "ids", "extent"): "ids defines B and S: fewer rows are a smaller legal call",
    ("embed_ln_bwd", "ids", "extent"): "ids defines B and S: fewer rows are a smaller legal call",
    ("embed_ln_fwd", "typ", "extent"): "typ defines the type vocabulary; the kernel clamps type ids against it",
    ("embed_ln_bwd", "typ", "extent"): "as embed_ln_fwd: typ defines the type vocabulary, and gtyp is checked against it",
    ("colsum", "x", "extent"): "x defines rows and cols unless rows= / cols= say otherwise: the count cases cover it",
    ("softmax_xent", "logits", "extent"): "logits defines rows and C unless rows= / C= say otherwise: the count cases cover it",
    ("sigmoid_xent", "logits", "extent"): "logits defines rows and C: a smaller logits is a smaller legal call",
    ("argmax", "x", "extent"): "x defines rows and C unless rows= / C= say otherwise: the count cases cover it",
    ("adam_step", "p", "extent"): "p defines n; the windows the kernel walks live in the device table seg, which the host cannot read",
    ("sqnorm", "g", "extent"): "g defines n: a shorter g is a smaller legal call",
    ("sqnorm_segments", "g", "extent"): "the windows of g that are read live in the device table seg, which the host cannot read",
    ("clip_scale", "sq", "extent"): "sq defines the number of terms: a shorter sq is a smaller legal call",
    ("scale_", "x", "extent"): "x defines n: a shorter x is a smaller legal call",
    ("transpose_bf16_batched", "src_base", "extent"): "the offsets into the arena live in the device table segs_dev; dst_base is checked against src_base",
    ("set_dynamic_params", "block", "dtype"): "16 raw bytes {u32, f32, f32, u32}: any dtype that holds them is legal",
    ("centroid_scores", "codes", "extent"): "codes defines N and Ld: fewer rows are a smaller corpus, and score is checked against that N",
    ("centroid_scores_ids", "codes", "extent"): "codes defines N and Ld: the kernel gives -inf to a candidate outside that N",
    ("centroid_codes", "sim", "extent"): "sim defines rows and K unless rows= / K= say otherwise: the count cases cover it",
    ("ivf_count", "codes", "extent"): "codes defines N and Ld: fewer rows are a smaller corpus",
    ("ivf_fill", "codes", "extent"): "codes defines N and Ld: fewer rows are a smaller corpus",
    ("ivf_fill", "docs", "extent"): "the extent written is offsets[K], which lives on the device; the kernel never stores past docs' own length",
    ("ivf_mark", "offsets", "extent"): "offsets defines K: a shorter table is a smaller codebook, and a probe past it is skipped",
    ("ivf_mark", "docs", "extent"): "the extent read is offsets[K], which lives on the device; the kernel never reads past docs' own length",
    ("ivf_compact", "count", "extent"): "count defines B: a shorter count is a smaller legal call",
}


def op_of(key):
    return key.split(":")[0]


def param_of(path):
    return path.split("[")[0].split(".")[0]


# ------------------------------------------------------------------------------------------------- reaching into the arguments
_FIELD = {"dy": 0, "x": 1, "dw": 2, "db": 3}


def get(p, path):
    if "[" not in path:
        return p[path]
    name, rest = path.split("[")
    k, field = rest.split("].")
    return p[name][int(k)][_FIELD[field]]


def put(p, path, value):
    if "[" not in path:
        p[path] = value
        return
    name, rest = path.split("[")
    k, field = rest.split("].")
    items = [list(q) for q in p[name]]
    items[int(k)][_FIELD[field]] = value
    p[name] = [tuple(q) for q in items]


def tensor_paths(key):
    return list(CASES[key].tensors)


def map_tensors(p, fn):
    """A copy of the arguments with fn applied to every tensor (those inside `problems` included)."""
    out = {}
    for k, v in p.items():
        if torch.is_tensor(v):
            out[k] = fn(v)
        elif isinstance(v, list):
            out[k] = [tuple(fn(t) if torch.is_tensor(t) else t for t in q) for q in v]
        else:
            out[k] = v
    return out


# ------------------------------------------------------------------------------------------------- mutations
def strided_inner(t):
    """The same values and shape with an inner stride of 2."""
    big = torch.zeros(*t.shape[:-1], t.shape[-1] * 2, dtype=t.dtype, device=t.device)
    v = big[..., ::2]
    v.copy_(t)
    return v


def row_padded(t):
    """The same values and shape as rows of a wider buffer: unit inner stride, not contiguous."""
    big = torch.zeros(*t.shape[:-1], t.shape[-1] + 3, dtype=t.dtype, device=t.device)
    v = big[..., :t.shape[-1]]
    v.copy_(t)
    return v


class Bad:
    def __init__(self, key, family, path, what, mutate, names):
        self.key, self.family, self.path, self.what, self.mutate, self.names = key, family, path, what, mutate, tuple(names)
        self.op = op_of(key)
        self.id = f"{key}-{family}-{path}-{what}"

    def args(self, place=lambda t: t):
        """The bad call's arguments; `place` moves good()'s tensors first (to the device, for the GPU test)."""
        p = map_tensors(CASES[self.key].good(), place)
        self.mutate(p)
        return p


def _on(path, fn):
    def mutate(p):
        put(p, path, fn(get(p, path)))
    return mutate


def _set(name, value):
    def mutate(p):
        p[name] = value
    return mutate


def _overlapping(a, b):
    """a and b as the two shifted views buf[1:] and buf[:-1] of one allocation; b keeps its values."""
    def mutate(p):
        t = p[b]
        buf = torch.zeros(t.shape[0] + 1, *t.shape[1:], dtype=t.dtype, device=t.device)
        buf[:-1].copy_(t)
        p[b], p[a] = buf[:-1], buf[1:]
    return mutate


def bad_cases(families=("dtype", "extent", "layout", "count", "overlap", "device")):
    out = []
    for key, case in CASES.items():
        good = case.good()
        for path, spec in case.tensors.items():
            t = get(good, path)
            names = (param_of(path),) + spec.blame
            if "dtype" in families and spec.bad is not None:
                out.append(Bad(key, "dtype", path, str(spec.bad).replace("torch.", ""), _on(path, lambda t, d=spec.bad: t.to(d)), names))
            if "extent" in families:
                for e in spec.ext:
                    if e == "row":
                        out.append(Bad(key, "extent", path, "row", _on(path, lambda t: t[:-1]), names))
                    elif t.dim() >= 2:
                        out.append(Bad(key, "extent", path, "col", _on(path, lambda t: t[:, :-1]), names))
            if "layout" in families and spec.layout is not None and t.shape[-1] > 1:
                out.append(Bad(key, "layout", path, "inner_stride", _on(path, strided_inner), names))
                if spec.layout == "flat" and t.dim() >= 2 and t.shape[0] > 1:
                    out.append(Bad(key, "layout", path, "row_padded", _on(path, row_padded), names))
            if "device" in families:
                out.append(Bad(key, "device", path, "host", _on(path, lambda t: t.cpu()), names))
        if "count" in families:
            for name, value, names in case.counts:
                out.append(Bad(key, "count", name, str(value), _set(name, value), names))
        if "overlap" in families:
            for a, b in case.overlaps:
                out.append(Bad(key, "overlap", a, b, _overlapping(a, b), (a, b)))
    return out


def shape_and_engine_dtype_cases():
    """For the retrieval wrappers, the two mistakes that used to surface from elsewhere (a ValueError from unpacking a
    shape, `unsupported dtype` from the dtype table): every tensor of two or more dimensions given with one dimension
    fewer (t[0]), and every f32-or-bf16 tensor given as f16 and as f64.  Refused by name like every other bad call."""
    out = []
    for key, case in CASES.items():
        if op_of(key) not in RETRIEVAL_OPS:
            continue
        good = case.good()
        for path, spec in case.tensors.items():
            names = (param_of(path),) + spec.blame
            if get(good, path).dim() >= 2:
                out.append(Bad(key, "dims", path, "one_fewer", _on(path, lambda t: t[0]), names))
            if spec.bad in (BF16, F64):
                for d in (torch.float16, F64):
                    out.append(Bad(key, "dtype", path, str(d).replace("torch.", ""), _on(path, lambda t, d=d: t.to(d)), names))
    return out


def covered(family):
    """{(wrapper, parameter)} with at least one generated bad case of the family."""
    return {(b.op, param_of(b.path)) for b in bad_cases((family,))}


def check_refused(ops, bad, args, rec):
    """The bad call raises before anything is recorded.  A host tensor is refused by the shared device check with a
    PolusHipError; every other refusal starts with the wrapper and a blamed parameter."""
    import re
    from polus_amd._lib import PolusHipError
    try:
        getattr(ops, bad.op)(**args)
    except (AssertionError, PolusHipError) as e:
        err = e
    else:
        raise AssertionError(f"{bad.id}: not refused (reached {rec.names()})")
    assert rec.calls == [], f"{bad.id}: reached {rec.names()} before the refusal"
    if bad.family == "device":
        assert isinstance(err, PolusHipError), f"{bad.id}: {err!r}"
        return
    m = re.match(rf"{re.escape(bad.op)}: (\w+)", str(err))
    assert m and m.group(1) in bad.names, f"{bad.id}: the refusal must start with '{bad.op}: <one of {bad.names}>', got: {err}"
