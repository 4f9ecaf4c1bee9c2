"""The contract between a caller and the training-step wrappers of polus_amd/ops.py, stated once.

The kernels take raw pointers, so a wrapper is the only place that can see a tensor's dtype, length and strides.  For every
wrapper of CORE_OPS this table holds

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
flat pointer and a count), "count", and "device" (a host tensor).  A bad call must raise AssertionError or PolusHipError
before any entry point is reached, and the message must start with "<wrapper>: <parameter>" naming the mutated parameter or
one of the parameters its spec blames (the partner of a mismatch).  The device family keeps the shared `_req_cuda`, whose
message names neither.

Where the header makes a looser form legal the table says so instead of refusing it: embed_ln_fwd takes f32 tables with a
bf16 y (tables are f32 whatever the engine's dtype), and gemm / dense_thin take an f32 output or gradient beside bf16
operands.  Needs no GPU to import."""
import inspect

import numpy as np
import torch

F32, BF16, I32, I64, F64 = torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.float64
SWAP = {F32: BF16, BF16: F32, I32: I64, I64: I32}
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

# every other public function of ops.py: the retrieval wrappers, the host-only route reports and the helpers
OTHER_OPS = ("workspace", "set_env", "reserve_cus", "gemm_route", "dense_bwd_params_route", "dense_bwd_params_grouped_route",
             "rowwise_route", "layernorm_bwd_partial_floats", "softmax_xent_wide_route", "softmax_xent_wide", "gather_rows",
             "inverse_map", "crf_nll", "crf_viterbi", "maxsim_fwd", "maxsim_scores", "maxsim_rerank", "fp8_quantize",
             "fp8_dequantize", "maxsim_scores_fp8", "maxsim_rerank_fp8", "residual_compress", "residual_decompress",
             "maxsim_rerank_res", "topk_merge", "centroid_scores_route", "centroid_scores", "centroid_codes", "centroid_update",
             "centroid_scores_ids", "ivf_count", "ivf_offsets", "ivf_fill", "ivf_mark", "ivf_compact", "splade_pool_fwd",
             "splade_pool_bwd", "flops_reg", "sparse_scores", "bm25_term_counts", "bm25_weights", "bm25_query",
             "postings_count", "postings_offsets", "postings_fill", "sparse_compact_rows", "bm25_query_lists",
             "postings_scores", "mine_negatives", "fuse_lists", "maxsim_bwd", "l2norm_fwd", "l2norm_bwd", "maxsim_tuples_fwd",
             "maxsim_tuples_bwd", "dot_tuples_fwd", "dot_tuples_bwd", "distill_kl", "margin_mse", "pair_lengths", "pair_pack",
             "pair_scatter_scores", "bio_entity_counts", "bio_spans", "dense_thin_supported", "dropout_mask")


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
    def __init__(self, good, entry, tensors, scalars=(), counts=(), expect=None):
        self.good, self.entry, self.tensors, self.scalars, self.counts, self.expect = good, tuple(entry), tensors, tuple(scalars), tuple(counts), expect


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


def bad_cases(families=("dtype", "extent", "layout", "count", "device")):
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
