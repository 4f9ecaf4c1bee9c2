"""CPU: the wrappers of the training step and of token retrieval (polus_amd/ops.py, CORE_OPS and RETRIEVAL_OPS of
tests/ops_contract_cases.py) hand the library what
the table expects for a legal call and refuse every generated illegal one before any entry point is reached, and the C entry
points behind them refuse by name what they can see from the host.

The wrappers run against tests.fakes.RecordingLib, a proxy over the real in-tree library that records instead of launching;
no bad call ever reaches the real library."""
import ctypes
import inspect

import pytest
import torch

from tests import ops_contract_cases as oc
from tests.fakes import disable_device_check, recording_lib


@pytest.fixture(scope="module")
def real_lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


@pytest.fixture
def rec(real_lib, monkeypatch):
    """The recording library installed, a dummy stream handle cached (so ops._st() needs no device), fresh workspaces."""
    yield from recording_lib(real_lib, monkeypatch, oc.STREAM)


@pytest.fixture
def no_device_check(monkeypatch):
    disable_device_check(monkeypatch)


# ------------------------------------------------------------------------------------------------- the table itself
def test_every_public_function_of_ops_is_classified():
    from polus_amd import ops
    public = oc.public_functions(ops)
    tabled = oc.CORE_OPS + oc.RETRIEVAL_OPS
    assert not set(tabled) & set(oc.OTHER_OPS) and not set(oc.CORE_OPS) & set(oc.RETRIEVAL_OPS)
    assert sorted(tabled + oc.OTHER_OPS) == public, (
        f"unclassified: {sorted(set(public) - set(tabled) - set(oc.OTHER_OPS))}, "
        f"gone: {sorted(set(tabled + oc.OTHER_OPS) - set(public))}")
    assert sorted({oc.op_of(k) for k in oc.CASES}) == sorted(tabled)


def test_every_tensor_parameter_has_a_dtype_and_an_extent_case(real_lib):
    from polus_amd import ops
    have = {fam: oc.covered(fam) for fam in ("dtype", "extent")}
    for op in oc.CORE_OPS + oc.RETRIEVAL_OPS:
        keys = [k for k in oc.CASES if oc.op_of(k) == op]
        tensors = {oc.param_of(path) for k in keys for path in oc.CASES[k].tensors}
        for k in keys:
            case = oc.CASES[k]
            scalars = set(case.scalars) | {c[0] for c in case.counts}
            params = list(inspect.signature(getattr(ops, op)).parameters)
            good = case.good()
            assert set(good) <= set(params), (k, set(good) - set(params))
            for name in params:
                mine = {oc.param_of(path) for path in case.tensors}
                assert (name in mine) != (name in scalars), f"{k}: parameter {name} must be either a tensor of the table or a listed scalar"
                if name in scalars:
                    assert not torch.is_tensor(good.get(name)), (k, name)
        for name in sorted(tensors):
            for fam in ("dtype", "extent"):
                reason = oc.EXEMPT.get((op, name, fam))
                if (op, name) in have[fam]:
                    assert reason is None, f"{op}.{name} has a {fam} case and an exemption"
                else:
                    assert isinstance(reason, str) and len(reason) > 10, f"{op}.{name}: no {fam} case and no reason in EXEMPT"
    for (op, name, fam), reason in oc.EXEMPT.items():
        assert op in oc.CORE_OPS + oc.RETRIEVAL_OPS and fam in ("dtype", "extent") and isinstance(reason, str) and reason, (op, name, fam)


# ------------------------------------------------------------------------------------------------- good calls
@pytest.mark.parametrize("key", list(oc.CASES))
def test_good_call_reaches_its_entry_points_with_the_expected_arguments(key, rec, no_device_check):
    from polus_amd import ops
    case = oc.CASES[key]
    args = case.good()
    getattr(ops, oc.op_of(key))(**args)
    assert tuple(rec.names()) == case.entry
    expected = case.expect(args)
    for name, got in rec.calls:
        want = expected[name]
        assert len(got) == len(want), (name, len(got), len(want))
        for k, (g, w) in enumerate(zip(got, want)):
            assert w == g, f"{key}: argument {k} of {name} is {g!r}, the table expects {w!r}"


def test_grouped_problem_table_holds_the_expected_pointers(rec, no_device_check):
    from polus_amd import ops
    args = oc.CASES["dense_bwd_params_grouped"].good()
    ops.dense_bwd_params_grouped(**args)
    arr = rec.calls[0][1][2]
    for q, (dy, x, dw, db) in zip(arr, args["problems"]):
        assert (q.dY, q.lddy, q.X, q.ldx, q.dW, q.lddw, q.db, q.n_out, q.n_in) == (
            dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dw.data_ptr(), dw.stride(0), db.data_ptr(), dy.shape[1], x.shape[1])


# ------------------------------------------------------------------------------------------------- bad calls
BAD = oc.bad_cases(("dtype", "extent", "layout", "count", "overlap"))


@pytest.mark.parametrize("bad", BAD, ids=[b.id for b in BAD])
def test_bad_call_is_refused_by_name_before_any_entry_point(bad, rec, no_device_check):
    from polus_amd import ops
    oc.check_refused(ops, bad, bad.args(), rec)


SHAPE_DTYPE = oc.shape_and_engine_dtype_cases()


@pytest.mark.parametrize("bad", SHAPE_DTYPE, ids=[b.id for b in SHAPE_DTYPE])
def test_retrieval_wrappers_name_a_wrong_dimension_count_and_a_wrong_engine_dtype(bad, rec, no_device_check):
    from polus_amd import ops
    oc.check_refused(ops, bad, bad.args(), rec)


def test_one_column_scores_are_legal_in_the_maxsim_wrappers(rec, no_device_check):
    """A [B, 1] column view of a wider matrix has an inner stride that no kernel ever steps by: legal, as in every
    other wrapper, and its row stride is what the library is handed."""
    from polus_amd import ops
    for key, name in (("maxsim_fwd", "score"), ("maxsim_scores", "score"), ("maxsim_bwd", "dscore")):
        args = oc.CASES[key].good()
        one = {"d": lambda t: t[:1], "dmask": lambda t: t[:1], "argmax": lambda t: t[:, :1].contiguous(), "dd": lambda t: t[:1]}   # N = 1
        args.update({k: cut(args[k]) for k, cut in one.items() if k in args})
        args[name] = torch.zeros(oc.R_B, 6)[:, ::3][:, :1]                      # [B, 1] with strides (6, 3)
        assert args[name].stride() == (6, 3)
        rec.calls.clear()
        getattr(ops, key)(**args)
        (fn, got), = rec.calls
        k = got.index(args[name].data_ptr())
        assert got[k + 1] == 6 and oc.R_B in got and 1 in got, (key, fn, got)


@pytest.mark.parametrize("key", list(oc.CASES))
def test_host_tensors_are_refused_by_the_real_device_check(key, rec):
    from polus_amd import ops
    from polus_amd._lib import PolusHipError
    with pytest.raises(PolusHipError):
        getattr(ops, oc.op_of(key))(**oc.CASES[key].good())
    assert rec.calls == []


def test_every_core_wrapper_states_its_contract():
    from polus_amd import ops
    for op in oc.CORE_OPS + oc.RETRIEVAL_OPS:
        doc = inspect.getdoc(getattr(ops, op))
        assert doc and len(doc) > 40, f"{op} has no docstring stating its contract"


# ------------------------------------------------------------------------------------------------- the C entry points behind them
def test_core_entry_points_refuse_by_name(real_lib):
    """Every refusal of the entry points of loss.hip, norm.hip, embed.hip, optim.hip, runtime.hip, attention.hip and
    dense_thin.hip that depends on host-visible arguments alone: a non-zero return and the distinguishing words of its
    message.  Dummy pointers: a refusal comes before any launch, and only calls with one bad argument are made."""
    lib = real_lib
    p, q = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)      # 16-byte aligned; 4 bytes off
    BIG = 1 << 40                                                          # workspace_bytes no entry point finds too small
    made = []

    def entry(fn, order, **defaults):
        def call(msg, **kw):
            assert kw, "only bad calls are made: a legal one would launch on the dummy pointers"
            args = dict(defaults, **kw)
            rc = getattr(lib, fn)(*[args[k] for k in order.split()])
            err = lib.polus_last_error()
            assert rc != 0 and err.startswith(fn.encode()) and msg in err, (fn, kw, rc, err)
            made.append(fn)
        return call

    # ---- loss.hip
    c = entry("polus_softmax_xent", "dtype logits ldl labels cw loss d lddl rows C ws wsb st", dtype=0, logits=p, ldl=3, labels=p, cw=None,
              loss=p, d=p, lddl=3, rows=4, C=3, ws=p, wsb=BIG, st=None)
    for kw in (dict(logits=None), dict(labels=None), dict(loss=None), dict(d=None)):
        c(b"null pointer", **kw)
    for kw in (dict(rows=0), dict(C=0), dict(ldl=2), dict(lddl=2)):
        c(b"bad shape", **kw)
    c(b"workspace too small", ws=None)
    c(b"workspace too small", wsb=4)
    c(b"bad dtype", dtype=7)
    c = entry("polus_sigmoid_xent", "dtype logits ldl y ldy cw nw loss d lddl rows C ws wsb st", dtype=0, logits=p, ldl=3, y=p, ldy=3, cw=p,
              nw=0.5, loss=p, d=p, lddl=3, rows=4, C=3, ws=p, wsb=BIG, st=None)
    for kw in (dict(logits=None), dict(y=None), dict(cw=None), dict(loss=None), dict(d=None)):
        c(b"null pointer", **kw)
    for kw in (dict(rows=0), dict(C=0), dict(ldl=2), dict(lddl=2), dict(ldy=2)):
        c(b"bad shape", **kw)
    c(b"workspace too small", ws=None)
    c(b"bad dtype", dtype=7)
    c = entry("polus_confusion_matrix", "r c n C cm rej st", r=p, c=p, n=6, C=3, cm=p, rej=None, st=None)
    for kw in (dict(r=None), dict(c=None), dict(cm=None), dict(n=-1), dict(C=0), dict(C=129)):
        c(b"0 < C <= 128", **kw)
    c = entry("polus_argmax", "x ldx out rows C st", x=p, ldx=3, out=p, rows=4, C=3, st=None)
    for kw in (dict(x=None), dict(out=None), dict(rows=0), dict(C=0), dict(ldx=2)):
        c(b"polus_argmax: bad arguments", **kw)
    c = entry("polus_crf_nll", "dtype pot tags len trans sw loss dpot dtrans acc B S C ws wsb st", dtype=0, pot=p, tags=p, len=None, trans=p,
              sw=None, loss=p, dpot=p, dtrans=p, acc=0, B=2, S=3, C=4, ws=p, wsb=BIG, st=None)
    for kw in (dict(pot=None), dict(tags=None), dict(trans=None), dict(loss=None), dict(dpot=None), dict(dtrans=None)):
        c(b"polus_crf_nll: null pointer", **kw)
    for kw in (dict(B=0), dict(S=0), dict(C=0), dict(C=100000)):
        c(b"need 0 < C <=", **kw)
    c(b"workspace too small", ws=None)
    c(b"bad dtype", dtype=7)
    c = entry("polus_crf_viterbi", "pot len trans out B S C ws wsb st", pot=p, len=None, trans=p, out=p, B=2, S=3, C=4, ws=p, wsb=BIG, st=None)
    for kw in (dict(pot=None), dict(trans=None), dict(out=None)):
        c(b"polus_crf_viterbi: null pointer", **kw)
    for kw in (dict(B=0), dict(C=0), dict(C=100000)):
        c(b"need 0 < C <=", **kw)
    c(b"workspace too small", wsb=4)

    # ---- norm.hip
    r = (ctypes.c_int * 7)()
    c = entry("polus_rowwise_route", "dtype rows H det out", dtype=0, rows=5, H=4, det=0, out=r)
    c(b"bad dtype 7", dtype=7)
    for kw in (dict(rows=0), dict(H=6), dict(H=0), dict(H=2052), dict(out=None)):
        c(b"polus_rowwise_route: bad arguments", **kw)
    c = entry("polus_layernorm_fwd", "dtype x g b y mean rstd rows H eps st", dtype=0, x=p, g=p, b=p, y=p, mean=p, rstd=p, rows=5, H=4,
              eps=1e-12, st=None)
    for kw in (dict(x=None), dict(g=None), dict(b=None), dict(y=None), dict(mean=None), dict(rstd=None)):
        c(b"polus_layernorm_fwd: null pointer", **kw)
    for kw in (dict(H=6), dict(H=0), dict(H=2052), dict(rows=0)):
        c(b"must be a multiple of 4", **kw)
    for kw in (dict(x=q), dict(y=q), dict(g=q), dict(b=q)):
        c(b"16-byte aligned", **kw)
    c(b"polus_layernorm_fwd: bad dtype", dtype=7)
    c = entry("polus_layernorm_bwd", "dtype dy x g mean rstd dx dg db dbias acc rows H dxm p seed ws wsb st", dtype=0, dy=p, x=p, g=p, mean=p,
              rstd=p, dx=p, dg=p, db=p, dbias=None, acc=0, rows=5, H=4, dxm=None, p=0.0, seed=0, ws=p, wsb=BIG, st=None)
    for kw in (dict(dy=None), dict(x=None), dict(g=None), dict(mean=None), dict(rstd=None), dict(dx=None), dict(dg=None), dict(db=None)):
        c(b"polus_layernorm_bwd: null pointer", **kw)
    for kw in (dict(p=1.0, dxm=p), dict(p=-0.1, dxm=p)):
        c(b"bad dropout arguments", **kw)
    c(b"dropout needs dx_masked", p=0.1)
    for kw in (dict(H=6), dict(H=2052), dict(rows=0)):
        c(b"polus_layernorm_bwd: bad H", **kw)
    for kw in (dict(x=q), dict(dy=q), dict(dx=q), dict(g=q)):
        c(b"16-byte aligned", **kw)
    c(b"polus_layernorm_bwd: workspace", ws=None)
    c(b"polus_layernorm_bwd: workspace", wsb=16)
    c(b"polus_layernorm_bwd: bad dtype", dtype=7)
    c = entry("polus_layernorm_bwd_finalize", "ws wsb rows H dg db dbias acc st", ws=p, wsb=BIG, rows=5, H=4, dg=p, db=p, dbias=None, acc=0, st=None)
    for kw in (dict(ws=None), dict(dg=None), dict(db=None), dict(rows=0), dict(H=0), dict(H=6)):
        c(b"polus_layernorm_bwd_finalize: bad arguments", **kw)
    c(b"polus_layernorm_bwd_finalize: workspace", wsb=16)
    c = entry("polus_colsum", "dtype x ldx rows cols out acc ws wsb st", dtype=0, x=p, ldx=6, rows=5, cols=6, out=p, acc=0, ws=p, wsb=BIG, st=None)
    for kw in (dict(x=None), dict(out=None), dict(rows=0), dict(cols=0), dict(ldx=5)):
        c(b"polus_colsum: bad arguments", **kw)
    c(b"polus_colsum: bad dtype", dtype=7)
    c(b"polus_colsum: workspace", ws=None)
    c(b"polus_colsum: workspace", wsb=8)

    # ---- embed.hip
    c = entry("polus_embed_ln_fwd", "dtype ids tt word pos typ g b y mean rstd B S H V P T eps p seed st", dtype=0, ids=p, tt=None, word=p, pos=p,
              typ=p, g=p, b=p, y=p, mean=p, rstd=p, B=2, S=3, H=4, V=7, P=3, T=2, eps=1e-12, p=0.0, seed=0, st=None)
    for kw in (dict(ids=None), dict(word=None), dict(pos=None), dict(typ=None), dict(g=None), dict(b=None), dict(y=None), dict(mean=None),
               dict(rstd=None)):
        c(b"polus_embed_ln_fwd: null pointer", **kw)
    for kw in (dict(p=1.0), dict(p=-0.5)):
        c(b"polus_embed_ln_fwd: bad drop_p", **kw)
    for kw in (dict(S=4), dict(B=0), dict(S=0)):
        c(b"exceeds max_position_embeddings", **kw)
    for kw in (dict(H=6), dict(H=2052), dict(V=0), dict(T=0)):
        c(b"polus_embed_ln_fwd: bad H", **kw)
    for kw in (dict(word=q), dict(pos=q), dict(typ=q), dict(y=q), dict(g=q), dict(b=q)):
        c(b"16-byte aligned", **kw)
    c(b"polus_embed_ln_fwd: bad dtype", dtype=7)
    c = entry("polus_embed_ln_bwd", "dtype dy ids tt word pos typ g mean rstd gw gp gt gg gb acc det B S H V P T p seed ws wsb st", dtype=0, dy=p,
              ids=p, tt=None, word=p, pos=p, typ=p, g=p, mean=p, rstd=p, gw=p, gp=p, gt=p, gg=p, gb=p, acc=0, det=0, B=2, S=3, H=4, V=7, P=3,
              T=2, p=0.0, seed=0, ws=p, wsb=BIG, st=None)
    for k in "dy ids word pos typ g mean rstd gw gp gt gg gb".split():
        c(b"polus_embed_ln_bwd: null pointer", **{k: None})
    c(b"polus_embed_ln_bwd: bad drop_p", p=1.0)
    for kw in (dict(B=0), dict(S=4), dict(H=6), dict(H=2052)):
        c(b"polus_embed_ln_bwd: bad shape", **kw)
    for kw in (dict(dy=q), dict(gw=q), dict(ws=q)):
        c(b"16-byte aligned", **kw)
    c(b"polus_embed_ln_bwd: workspace", ws=None)
    c(b"polus_embed_ln_bwd: workspace", wsb=16)
    c(b"polus_embed_ln_bwd: bad dtype", dtype=7)

    # ---- optim.hip
    c = entry("polus_adam_step", "p g m v sh seg nseg n lr lrt b1 b2 eps wd gs clip st", p=p, g=p, m=p, v=p, sh=None, seg=p, nseg=2, n=8, lr=1e-2,
              lrt=1e-2, b1=0.9, b2=0.999, eps=1e-7, wd=0.0, gs=1.0, clip=None, st=None)
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(seg=None), dict(nseg=0), dict(n=0)):
        c(b"polus_adam_step: bad arguments", **kw)
    for kw in (dict(p=q), dict(g=q), dict(m=q), dict(v=q)):
        c(b"16-byte aligned", **kw)
    c(b"shadow must be 8-byte aligned", sh=q)
    c = entry("polus_sqnorm", "g n out ws wsb st", g=p, n=9, out=p, ws=p, wsb=BIG, st=None)
    for kw in (dict(g=None), dict(out=None), dict(n=0), dict(g=q)):
        c(b"polus_sqnorm: bad arguments", **kw)
    c(b"polus_sqnorm: workspace too small", ws=None)
    c(b"polus_sqnorm: workspace too small", wsb=2)
    c = entry("polus_sqnorm_segments", "g seg nseg out ws wsb st", g=p, seg=p, nseg=2, out=p, ws=p, wsb=4096, st=None)
    for kw in (dict(g=None), dict(seg=None), dict(out=None), dict(nseg=0)):
        c(b"polus_sqnorm_segments: bad arguments", **kw)
    c(b"polus_sqnorm_segments: workspace too small", ws=None)
    c(b"polus_sqnorm_segments: workspace too small", wsb=4095)
    c = entry("polus_clip_scale", "sq n gs clip out st", sq=p, n=2, gs=1.0, clip=1.0, out=p, st=None)
    for kw in (dict(sq=None), dict(out=None), dict(clip=0.0), dict(n=0)):
        c(b"polus_clip_scale: bad arguments", **kw)

    # ---- runtime.hip
    assert lib.polus_set_dynamic_params(q) != 0 and b"16-byte aligned" in lib.polus_last_error()
    c = entry("polus_cast", "sd src dd dst n st", sd=0, src=p, dd=1, dst=p, n=8, st=None)
    for kw in (dict(src=None), dict(dst=None), dict(n=-1)):
        c(b"polus_cast: bad arguments", **kw)
    for kw in (dict(src=q), dict(sd=1, dd=0, dst=q)):
        c(b"4-element aligned", **kw)
    for kw in (dict(sd=7), dict(dd=7)):
        c(b"polus_cast: bad dtypes", **kw)
    c = entry("polus_scale", "x a n st", x=p, a=0.5, n=8, st=None)
    for kw in (dict(x=None), dict(n=-1)):
        c(b"polus_scale: bad arguments", **kw)
    c(b"16-byte aligned", x=q)
    c = entry("polus_act_bwd", "dtype dy u du n act st", dtype=0, dy=p, u=p, du=p, n=8, act=1, st=None)
    for kw in (dict(dy=None), dict(u=None), dict(du=None), dict(n=-1)):
        c(b"polus_act_bwd: bad arguments", **kw)
    for kw in (dict(dy=q), dict(u=q), dict(du=q)):
        c(b"4-element aligned", **kw)
    c(b"polus_act_bwd: bad dtype", dtype=7)
    c = entry("polus_transpose_bf16_batched", "src dst segs nseg tiles st", src=p, dst=p, segs=p, nseg=2, tiles=2, st=None)
    for kw in (dict(src=None), dict(dst=None), dict(segs=None), dict(nseg=0), dict(tiles=0)):
        c(b"polus_transpose_bf16_batched: bad arguments", **kw)
    for kw in (dict(src=q), dict(dst=q)):
        c(b"8-byte aligned", **kw)
    c = entry("polus_transpose_bf16", "src dst rows cols st", src=p, dst=p, rows=3, cols=4, st=None)
    for kw in (dict(src=None), dict(dst=None), dict(rows=0), dict(cols=0)):
        c(b"polus_transpose_bf16: bad arguments", **kw)
    c = entry("polus_dropout_mask", "seed p idx0 n mask st", seed=1, p=0.1, idx0=0, n=8, mask=p, st=None)
    for kw in (dict(mask=None), dict(n=-1), dict(p=1.0), dict(p=-0.1)):
        c(b"polus_dropout_mask: bad arguments", **kw)
    c = entry("polus_dropout", "dtype x y n p seed st", dtype=0, x=p, y=p, n=8, p=0.1, seed=1, st=None)
    for kw in (dict(x=None), dict(y=None), dict(n=-1), dict(n=1 << 32), dict(p=1.0), dict(p=-0.1)):
        c(b"polus_dropout: bad arguments", **kw)
    c(b"polus_dropout: bad dtype", dtype=7)

    # ---- attention.hip
    fwd, bwd = ctypes.c_int(), ctypes.c_int()
    c = entry("polus_attention_route", "dtype S fwd bwd", dtype=0, S=17, fwd=ctypes.byref(fwd), bwd=ctypes.byref(bwd))
    c(b"polus_attention_route: bad dtype", dtype=7)
    for kw in (dict(S=0), dict(fwd=None), dict(bwd=None)):
        c(b"polus_attention_route: bad arguments", **kw)
    shared = [(dict(dtype=7), b"bad dtype 7"), (dict(hd=32), b"head_dim must be 64"), (dict(B=0), b"bad shape"), (dict(S=0), b"bad shape"),
              (dict(A=0), b"bad shape"), (dict(B=65536), b"must be <= 65535"), (dict(A=65536), b"must be <= 65535"),
              (dict(qkv=None), b"null pointer"), (dict(ctx=None), b"null pointer"), (dict(lse=None), b"null pointer"),
              (dict(qkv=q), b"16-byte aligned"), (dict(ctx=q), b"16-byte aligned"), (dict(p=1.0), b"bad dropout arguments"),
              (dict(p=-0.1), b"bad dropout arguments"), (dict(p=0.1, B=4, A=16, S=8192), b"bad dropout arguments")]
    c = entry("polus_attention_fwd", "dtype qkv mask ctx lse B S A hd p seed st", dtype=0, qkv=p, mask=None, ctx=p, lse=p, B=1, S=17, A=1, hd=64,
              p=0.0, seed=0, st=None)
    for kw, msg in shared:
        c(msg, **kw)
    c = entry("polus_attention_bwd", "dtype qkv mask ctx dctx lse dqkv B S A hd p seed ws wsb st", dtype=0, qkv=p, mask=None, ctx=p, dctx=p, lse=p,
              dqkv=p, B=1, S=17, A=1, hd=64, p=0.0, seed=0, ws=p, wsb=BIG, st=None)
    for kw, msg in shared:
        c(msg, **kw)
    for kw in (dict(dctx=None), dict(dqkv=None)):
        c(b"polus_attention_bwd: null pointer", **kw)
    for kw in (dict(dctx=q), dict(dqkv=q)):
        c(b"16-byte aligned", **kw)
    c(b"polus_attention_bwd: workspace", ws=None)
    c(b"polus_attention_bwd: workspace", wsb=16)

    # ---- dense_thin.hip
    assert lib.polus_dense_thin_supported(7, 4, 3) == 0 and lib.polus_dense_thin_supported(0, 4, 9) == 0
    c = entry("polus_dense_thin_fwd", "dtype x ldx w ldw bias yd y ldy rows H C st", dtype=0, x=p, ldx=4, w=p, ldw=4, bias=None, yd=0, y=p, ldy=3,
              rows=5, H=4, C=3, st=None)
    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(rows=0)):
        c(b"polus_dense_thin_fwd: bad arguments", **kw)
    for kw in (dict(dtype=7), dict(C=9), dict(C=0), dict(H=6), dict(H=0), dict(H=2048)):
        c(b"polus_dense_thin_fwd: unsupported shape", **kw)
    c(b"y_dtype must be f32 or dtype", yd=1)
    for kw in (dict(x=q), dict(w=q), dict(ldx=5), dict(ldw=5)):
        c(b"16-byte aligned", **kw)
    c = entry("polus_dense_thin_bwd", "dtype x ldx dyd dy lddy w ldw dx lddx dw lddw db rows H C acc ws wsb st", dtype=0, x=p, ldx=4, dyd=0, dy=p,
              lddy=3, w=p, ldw=4, dx=p, lddx=4, dw=p, lddw=4, db=None, rows=5, H=4, C=3, acc=0, ws=p, wsb=BIG, st=None)
    for kw in (dict(x=None), dict(dy=None), dict(w=None), dict(dw=None), dict(rows=0)):
        c(b"polus_dense_thin_bwd: bad arguments", **kw)
    for kw in (dict(dtype=7), dict(C=9), dict(H=6), dict(H=2048)):
        c(b"polus_dense_thin_bwd: unsupported shape", **kw)
    c(b"dy_dtype must be f32 or dtype", dyd=1)
    for kw in (dict(x=q), dict(w=q), dict(dx=q), dict(ldx=5), dict(ldw=5), dict(lddx=5)):
        c(b"16-byte aligned", **kw)
    c(b"polus_dense_thin_bwd: workspace", ws=None)
    c(b"polus_dense_thin_bwd: workspace", wsb=16)
    assert len(set(made)) == 29, sorted(set(made))       # every entry point above (polus_set_dynamic_params is called directly)
