"""Cases for the GEMM family (gemm.hip, gemm_ring.hip, gemm_pp.hip, gemm_ppks.hip, dense_thin.hip), shared by the GPU
file that drives every route (test_gemm_views_gpu.py) and by the CPU check of the routing, of the exactness preconditions
and of the comparator (test_gemm_cases_cpu.py).  No GPU needed to import.

Framed views.  Every tensor handed to the library is a view inside a larger allocation, a Frame: GUARD rows above and
below, a leading dimension ld >= cols and a column offset.  Input frames are NaN outside the view, so padding that reaches
an output makes it non-finite.  Output frames hold SENTINEL outside the view, which must be bit-identical after the call;
inside, an output that is written starts as NaN and one that is accumulated into starts with integers.  The buffers are
always large enough for a correct kernel.

View kinds, each chosen for the host predicate it flips (es = element size in bytes):
  dense   ld = cols, offset 0
  pad16   ld = cols + 16 / es           every vector predicate stays true, ld != extent
  cls     ld = 3 * cols                 the h[:, 0, :] pattern of the pooler and of resid=d3[:, 0, :]
  pad4    bf16 C / resid / aux only, ld % 8 == 4: epi_vec true, epi_vec16 false
  pad1    ld = cols + 1                 every vector flag false
  shift1  ld as pad16, the view starts one element in: base pointer misaligned

Exact data.  A and B are drawn from {-1, 0, 1}, bias from the integers of [-8, 8], residual / prior C / the aux read by
relu' from [-16, 16]; alpha is 1 or 0.5, dropout p = 0.5 (scale exactly 2, threshold 32768), the activation relu.  Every
partial sum is a small integer or half-integer, exact in the f32 accumulator whatever the summation order, tiling or K
split, and the result is representable in bf16 (test_gemm_cases_cpu.py checks both per case).  So the device result must
equal the float64 reference bit for bit: check() compares with ==.  The gelu / swish / tanh cases cannot be exact: their
pre-activation written to aux still is, the activated output is held to tests.util.TOL of max|ref|.

The route a case expects is restated here from polus_amd/csrc/gemm.hip (gemm_plan's predicates, gemm_route, the grouped
dW plan) and held to the library by test_gemm_cases_cpu.py through the host-only route reports."""
import zlib
from dataclasses import dataclass

import numpy as np
import torch

from oracle import bert as ob
from tests.util import TOL, dropout_keep_np

GUARD = 4
SENTINEL = -1536.0            # finite, exact in bf16, outside every reference's range
ES = {"f32": 4, "bf16": 2}
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
NCU = 256                     # the MI355X's CU count; polus_num_cus() falls back to it without a device
DROP_P = 0.5
KINDS = ("dense", "pad16", "cls", "pad4", "pad1", "shift1")
OPERAND_KINDS = ("pad16", "cls", "pad1", "shift1")
EPI_KINDS = ("pad16", "cls", "pad4", "pad1", "shift1")
ACTS = {"relu": (lambda v: np.maximum(v, 0.0), lambda u: (u > 0).astype(np.float64)),
        "gelu": (ob.gelu, ob.gelu_grad), "swish": (ob.swish, ob.swish_grad),
        "tanh": (np.tanh, lambda u: 1.0 - np.tanh(u) ** 2)}

# epilogue families of polus_gemm: what the call passes.  aux: "w" written (ACT_FWD), "r" read (ACT_BWD)
EPI = {
    "plain": dict(),
    "bias": dict(bias=True),
    "alpha": dict(alpha=0.5, bias=True),
    "act_fwd": dict(bias=True, aux="w"),
    "resid": dict(bias=True, resid=True),
    "act_bwd": dict(aux="r"),
    "drop": dict(bias=True, resid=True, drop=True),
    "drop_only": dict(bias=True, drop=True),
    "accum": dict(alpha=0.5, bias=True, accum=True),
    "alpha_accum": dict(alpha=0.5, accum=True),
}


def geometry(kind, cols, es):
    """(ld, column offset) of a view kind."""
    if kind == "dense":
        return cols, 0
    if kind == "pad16":
        return cols + 16 // es, 0
    if kind == "cls":
        return 3 * cols, 0
    if kind == "pad4":
        return cols + ((4 - cols) % 8 or 8), 0
    if kind == "pad1":
        return cols + 1, 0
    if kind == "shift1":
        return cols + 16 // es, 1
    raise ValueError(kind)


class Frame:
    """One tensor of a call inside its allocation.  role: "in" (NaN outside), "write" (SENTINEL outside, NaN inside),
    "accum" (SENTINEL outside, `data` inside).  buf is float32 whatever the device dtype: every value put here is exact in
    bf16, and a bf16 result widens exactly."""

    def __init__(self, name, rows, cols, kind, dtype, role, data=None, vector=False):
        self.name, self.rows, self.cols, self.kind, self.dtype, self.role, self.vector = name, rows, cols, kind, dtype, role, vector
        self.ld, self.c0 = geometry(kind, cols, ES[dtype])
        assert self.ld >= self.c0 + cols
        self.buf = np.full((rows + 2 * GUARD, self.ld), np.nan if role == "in" else SENTINEL, np.float32)
        self.view[...] = np.nan if role == "write" else data

    @property
    def view(self):
        return self.buf[GUARD:GUARD + self.rows, self.c0:self.c0 + self.cols]

    @property
    def offset(self):
        """Elements from the start of the allocation to the view's first element."""
        return GUARD * self.ld + self.c0

    def inside(self):
        m = np.zeros(self.buf.shape, bool)
        m[GUARD:GUARD + self.rows, self.c0:self.c0 + self.cols] = True
        return m

    def view_of(self, buf):
        return buf[GUARD:GUARD + self.rows, self.c0:self.c0 + self.cols]

    def address(self, base=1 << 20):
        """A made-up address with the alignment the view has inside a 256-byte aligned allocation."""
        return base + self.offset * ES[self.dtype]


@dataclass
class Case:
    base: str                 # the route + epilogue + shape; the all-dense twin of a case is base + "/dense"
    op: str                   # gemm | dw | dwg | thin_fwd | thin_bwd
    dtype: str
    shape: tuple              # gemm (M, N, K); dw (T, n_out, n_in); dwg (T, ((n_out, n_in), ...)); thin (rows, H, C)
    want: str                 # the kernel the table expects of the all-dense variant
    c_dtype: str = None       # gemm: C; thin: y / dy
    layouts: tuple = (0, 0)
    epi: str = "plain"
    act: str = "relu"
    split_k: int = 1
    env: tuple = ()           # ((switch, value), ...)
    views: tuple = ()         # ((tensor, kind), ...); tensors not named are dense
    db: bool = True           # dw / dwg / thin_bwd: with the bias gradient
    accumulate: bool = False  # dw / dwg / thin_bwd
    refused: bool = False     # thin: the call must fail with PolusHipError and leave the outputs alone

    def __post_init__(self):
        if self.c_dtype is None:
            self.c_dtype = self.dtype if self.op == "gemm" else "f32"

    @property
    def tag(self):
        return "+".join(f"{t}={k}" for t, k in self.views) or "dense"

    @property
    def name(self):
        return f"{self.base}/{self.tag}"

    @property
    def exact(self):
        return self.act == "relu"

    @property
    def fast(self):
        return self.want not in ("v1", "fallback", "one_by_one", "thin")

    def kind(self, tensor):
        return dict(self.views).get(tensor, "dense")

    @property
    def seed(self):
        return zlib.crc32(self.base.encode())

    @property
    def drop_seed(self):
        return self.seed & 0xFFFF


# ------------------------------------------------------------------------------------------------ frames and references
def _ints(r, lo, hi, shape):
    return r.integers(lo, hi + 1, size=shape).astype(np.float32)


def build(case):
    """name -> Frame, inputs filled from the case's seed (the same data whatever the view kinds)."""
    r = np.random.Generator(np.random.PCG64(case.seed))
    f = {}

    def add(name, rows, cols, dtype, role, data=None, vector=False):
        f[name] = Frame(name, rows, cols, case.kind(name), dtype, role, data, vector)

    if case.op == "gemm":
        M, N, K = case.shape
        e = EPI[case.epi]
        add("A", *((M, K) if case.layouts[0] == 0 else (K, M)), case.dtype, "in", _ints(r, -1, 1, (M, K) if case.layouts[0] == 0 else (K, M)))
        add("B", *((N, K) if case.layouts[1] == 0 else (K, N)), case.dtype, "in", _ints(r, -1, 1, (N, K) if case.layouts[1] == 0 else (K, N)))
        prior = _ints(r, -16, 16, (M, N))
        add("C", M, N, case.c_dtype, "accum" if e.get("accum") else "write", prior)
        bias, resid, aux = _ints(r, -8, 8, (1, N)), _ints(r, -16, 16, (M, N)), _ints(r, -16, 16, (M, N))
        if e.get("bias"):
            add("bias", 1, N, "f32", "in", bias, vector=True)
        if e.get("resid"):
            add("resid", M, N, case.dtype, "in", resid)
        if e.get("aux") == "w":
            add("aux", M, N, case.dtype, "write")
        elif e.get("aux") == "r":
            add("aux", M, N, case.dtype, "in", aux if case.exact else aux / 4)     # quarters: where gelu' / swish' / tanh' move
    elif case.op in ("dw", "dwg"):
        T = case.shape[0]
        probs = [case.shape[1:]] if case.op == "dw" else case.shape[1]
        for k, (no, ni) in enumerate(probs):
            s = "" if case.op == "dw" else str(k)
            add("dY" + s, T, no, case.dtype, "in", _ints(r, -1, 1, (T, no)))
            add("X" + s, T, ni, case.dtype, "in", _ints(r, -1, 1, (T, ni)))
            add("dW" + s, no, ni, "f32", "accum" if case.accumulate else "write", _ints(r, -16, 16, (no, ni)))
            if case.db:
                add("db" + s, 1, no, "f32", "accum" if case.accumulate else "write", _ints(r, -16, 16, (1, no)), vector=True)
    elif case.op == "thin_fwd":
        rows, H, C = case.shape
        add("x", rows, H, case.dtype, "in", _ints(r, -1, 1, (rows, H)))
        add("w", C, H, case.dtype, "in", _ints(r, -1, 1, (C, H)))
        add("bias", 1, C, "f32", "in", _ints(r, -8, 8, (1, C)), vector=True)
        add("y", rows, C, case.c_dtype, "write")
    elif case.op == "thin_bwd":
        rows, H, C = case.shape
        add("x", rows, H, case.dtype, "in", _ints(r, -1, 1, (rows, H)))
        add("dy", rows, C, case.c_dtype, "in", _ints(r, -2, 2, (rows, C)))
        add("w", C, H, case.dtype, "in", _ints(r, -1, 1, (C, H)))
        add("dx", rows, H, case.dtype, "write")
        role = "accum" if case.accumulate else "write"
        add("dw", C, H, "f32", role, _ints(r, -16, 16, (C, H)))
        if case.db:
            add("db", 1, C, "f32", role, _ints(r, -16, 16, (1, C)), vector=True)
    else:
        raise ValueError(case.op)
    return f


def outputs(case, frames):
    return [n for n, fr in frames.items() if fr.role != "in"]


def keep_mask(case):
    M, N, _ = case.shape
    return dropout_keep_np(case.drop_seed, DROP_P, 0, M * N).reshape(M, N).astype(np.float64)


def reference(case, frames):
    """name -> float64 reference of every output view, from the frames' views."""
    v = {n: fr.view.astype(np.float64) for n, fr in frames.items()}
    ref = {}
    if case.op == "gemm":
        e = EPI[case.epi]
        a = v["A"] if case.layouts[0] == 0 else v["A"].T
        b = v["B"] if case.layouts[1] == 0 else v["B"].T
        x = e.get("alpha", 1.0) * (a @ b.T)
        if e.get("bias"):
            x = x + v["bias"]
        fwd, bwd = ACTS[case.act]
        if e.get("aux") == "w":
            ref["aux"] = x
            x = fwd(x)
        if e.get("aux") == "r":
            x = x * bwd(v["aux"])
        if e.get("drop"):
            x = x * keep_mask(case) * (1.0 / (1.0 - DROP_P))
        if e.get("resid"):
            x = x + v["resid"]
        if e.get("accum"):
            x = x + v["C"]
        ref["C"] = x
    elif case.op in ("dw", "dwg"):
        for s in ([""] if case.op == "dw" else [str(k) for k in range(len(case.shape[1]))]):
            ref["dW" + s] = v["dY" + s].T @ v["X" + s] + (v["dW" + s] if case.accumulate else 0.0)
            if case.db:
                ref["db" + s] = v["dY" + s].sum(0, keepdims=True) + (v["db" + s] if case.accumulate else 0.0)
    elif case.op == "thin_fwd":
        ref["y"] = v["x"] @ v["w"].T + v["bias"]
    elif case.op == "thin_bwd":
        ref["dx"] = v["dy"] @ v["w"]
        ref["dw"] = v["dy"].T @ v["x"] + (v["dw"] if case.accumulate else 0.0)
        if case.db:
            ref["db"] = v["dy"].sum(0, keepdims=True) + (v["db"] if case.accumulate else 0.0)
    return ref


def exact_outputs(case):
    """Outputs compared with ==: all of them on an exact case, the pre-activation on the others."""
    return None if case.exact else {"aux"}


def check(case, frames_after, reference):
    """The shared comparator.  frames_after: name -> the whole allocation (float32 array of the frame's shape) after the
    call, for every output.  Returns a list of findings, empty when the call did what the reference says and nothing
    else: every output view equal to the reference (== on exact cases, TOL of max|ref| on the activated output of the
    others), finite, and every byte outside the views as it was."""
    frames = build(case)
    findings = []
    for name in outputs(case, frames):
        fr, after = frames[name], np.asarray(frames_after[name], np.float32)
        if after.shape != fr.buf.shape:
            findings.append(f"{name}: frame shape {after.shape} != {fr.buf.shape}")
            continue
        out = ~fr.inside()
        moved = out & (after.view(np.uint32) != fr.buf.view(np.uint32))
        if moved.any():
            i, j = np.argwhere(moved)[0]
            findings.append(f"{name}: {int(moved.sum())} elements outside the view changed, first at frame row {i - GUARD} col {j - fr.c0} "
                            f"(view {fr.rows} x {fr.cols}, ld {fr.ld})")
        if case.refused:
            got = fr.view_of(after)              # a NaN may come back from bf16 with other payload bits: still a NaN, still unwritten
            if ((got.view(np.uint32) != fr.view.view(np.uint32)) & ~(np.isnan(got) & np.isnan(fr.view))).any():
                findings.append(f"{name}: a refused call wrote into the view")
            continue
        got, ref = fr.view_of(after).astype(np.float64), reference[name]
        bad = ~np.isfinite(got)
        if bad.any():
            i, j = np.argwhere(bad)[0]
            findings.append(f"{name}: {int(bad.sum())} non-finite elements, first at ({i}, {j})")
            continue
        if case.exact or name in exact_outputs(case):
            ne = got != ref
            if ne.any():
                i, j = np.argwhere(ne)[0]
                findings.append(f"{name}: {int(ne.sum())} of {ne.size} elements differ from the exact reference, first at ({i}, {j}): "
                                f"{got[i, j]!r} != {ref[i, j]!r}")
        else:
            err = float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))
            if not err <= TOL[DT[fr.dtype]]:
                findings.append(f"{name}: rel err {err:.3e} > {TOL[DT[fr.dtype]]:.1e}")
    return findings


# ------------------------------------------------------------------------------------------------ the expected routes
def _env(case, name, default):
    return int(dict(case.env).get(name, default))


def _pp_cus(case):
    return max(32, NCU - _env(case, "POLUS_GEMM_RESERVE_CUS", 0))


def _pp_tile(case, M, N, K, mode, vec16):
    sel = _env(case, "POLUS_GEMM_PP", 0)
    if sel < 0 or mode < 0 or K % 64 or M < 256 or N < 192 or not vec16:
        return 0
    if sel in (256, 192):
        return sel
    ncu, tm, best, best_tn = _pp_cus(case), (M + 255) // 256, 0.0, 0
    for tn in (256, 192):
        tiles = tm * ((N + tn - 1) // tn)
        rounds = (tiles + ncu - 1) // ncu
        score = M * N / (rounds * ncu * 256.0 * tn) * (1.10 if tn == 256 else 1.0)
        if score > best:
            best, best_tn = score, tn
    return best_tn if best >= 0.70 else 0


def _use_ring128(case, M, N, mode):
    sel = _env(case, "POLUS_GEMM_RING128", 0)
    if sel < 0 or mode < 0 or M < 128 or N < 128:
        return False
    return sel > 0 or 20 * ((M + 255) // 256) * ((N + 127) // 128) <= 11 * 2 * NCU


def _aligned(addr, n=16):
    return addr % n == 0


def gemm_route(dtype, c_dtype, layouts, M, N, K, split_k, ptrs, case, bias=False, resid=False, aux=None, drop=False, accum=False):
    """gemm_plan + gemm_route of polus_amd/csrc/gemm.hip restated.  ptrs: tensor -> (address, ld)."""
    es, ecs, epc = ES[dtype], ES[c_dtype], 16 // ES[dtype]
    (pa, lda), (pb, ldb), (pc, ldc) = ptrs["A"], ptrs["B"], ptrs["C"]
    a_vec = _aligned(pa) and lda * es % 16 == 0 and (K if layouts[0] == 0 else M) % epc == 0
    b_vec = _aligned(pb) and ldb * es % 16 == 0 and (K if layouts[1] == 0 else N) % epc == 0
    ev = pc % (4 * ecs) == 0 and ldc % 4 == 0
    ev16 = _aligned(pc) and ldc * ecs % 16 == 0
    if bias:
        ev, ev16 = ev and _aligned(ptrs["bias"][0]), ev16 and _aligned(ptrs["bias"][0])
    for t in (["resid"] if resid else []) + (["aux"] if aux else []):
        p, ld = ptrs[t]
        ev = ev and p % (4 * es) == 0 and ld % 4 == 0
        ev16 = ev16 and _aligned(p) and ld * es % 16 == 0
    ev16 = ev16 and dtype == "bf16"
    bk = 64 if dtype == "bf16" else 32
    nkt = (K + bk - 1) // bk
    split_k = min(max(split_k, 1), nkt)
    kt_per = (nkt + split_k - 1) // split_k
    splits = (nkt + kt_per - 1) // kt_per
    both_kc, c_f32 = layouts == (0, 0), c_dtype == "f32"
    epi = resid or aux is not None or drop
    fast = dtype == "bf16" and a_vec and b_vec and M >= 256 and N >= 128 and "POLUS_GEMM_V1" not in dict(case.env)
    r = dict(kernel="ring" if fast else "v1", tn=128, mode=-1, drop=int(drop), splits=splits, reduce="none", persist_cus=0,
             a_vec=a_vec, b_vec=b_vec, epi_vec=ev, epi_vec16=ev16)
    if splits > 1:
        if not epi:
            r["reduce"] = "plain"
        elif fast and both_kc and not c_f32:
            r["reduce"] = "epi"
        else:
            r["splits"] = 1
    if fast and r["splits"] == 1:
        if both_kc and not c_f32 and not accum:                       # epi_mode
            fwd, bwd = aux == "w", aux == "r"
            if not ((fwd and (resid or drop)) or (bwd and (resid or drop)) or (drop and not resid)):
                r["mode"] = 1 if fwd else 3 if bwd else 2 if resid else 0
        tn = _pp_tile(case, M, N, K, r["mode"], ev16)
        if tn:
            sel = _env(case, "POLUS_GEMM_PERSIST", 1)
            tiles = ((M + 255) // 256) * ((N + tn - 1) // tn)
            if sel and (tn == 256 or sel >= 2) and tiles > _pp_cus(case):
                r["persist_cus"] = _pp_cus(case)
            r.update(tn=tn, kernel="pp_persist" if r["persist_cus"] else "pp")
        elif _use_ring128(case, M, N, r["mode"]):
            r["kernel"] = "ring128"
        elif drop:
            r["kernel"] = "ring_drop"
    r["v1_vec"] = r["kernel"] == "v1" and a_vec and b_vec
    return r


def _ptrs(frames, names):
    return {n: (frames[n].address(), frames[n].ld) for n in names if n in frames}


def _dw_single(case, dtype, T, no, ni, split_k, py, px, pw, db):
    """polus_dense_bwd_params: (ring, K slices)."""
    es = ES[dtype]
    vec = _aligned(py[0]) and _aligned(px[0]) and py[1] * es % 16 == 0 and px[1] * es % 16 == 0 and no % (16 // es) == 0 and ni % (16 // es) == 0
    if dtype == "bf16" and vec and no >= 256 and ni >= 128 and db and "POLUS_GEMM_V1" not in dict(case.env):
        nkt = (T + 63) // 64
        kt_per = (nkt + min(max(split_k, 1), nkt) - 1) // min(max(split_k, 1), nkt)
        return True, (nkt + kt_per - 1) // kt_per
    return False, gemm_route(dtype, "f32", (1, 1), no, ni, T, split_k, dict(A=py, B=px, C=pw), case)["splits"]


def _sk_plan(tiles, T, ncu, delta):
    """polus_ppks_sk_plan (gemm_ppks.hip): slots per tile of the stream-K hybrid, 0 where it does not apply."""
    if T % 64 or ncu < 8:
        return 0
    nkt, ttot = T // 64, sum(tiles)
    base = ncu // ttot
    R = ncu - base * ttot
    kr = (ttot * nkt + ncu - 1) // ncu + delta
    if base < 1 or R < 4 or kr < 4 or base * kr >= nkt or ttot * (nkt - base * kr) < R:
        return 0
    krem = nkt - base * kr
    q = ttot * krem // R
    return base + (krem + q - 1) // q + 1


def expected_route(case, frames):
    """What the library's route report must say for this case, as a dict with the report's field names."""
    if case.op == "gemm":
        e = EPI[case.epi]
        return gemm_route(case.dtype, case.c_dtype, case.layouts, *case.shape, case.split_k, _ptrs(frames, ("A", "B", "C", "bias", "resid", "aux")),
                          case, bias=e.get("bias", False), resid=e.get("resid", False), aux=e.get("aux"), drop=e.get("drop", False),
                          accum=e.get("accum", False))
    if case.op == "dw":
        T, no, ni = case.shape
        p = _ptrs(frames, ("dY", "X", "dW"))
        ring, splits = _dw_single(case, case.dtype, T, no, ni, case.split_k, p["dY"], p["X"], p["dW"], case.db)
        return dict(ring=ring, splits=splits)
    if case.op == "dwg":
        T, probs = case.shape
        env, es = dict(case.env), ES[case.dtype]
        P = [_ptrs(frames, (f"dY{k}", f"X{k}", f"dW{k}")) for k in range(len(probs))]
        ring = case.dtype == "bf16" and "POLUS_GEMM_V1" not in env and "POLUS_DW_UNGROUPED" not in env
        aligned = True
        for k, (no, ni) in enumerate(probs):
            (py, ldy), (px, ldx), (pw, ldw) = P[k][f"dY{k}"], P[k][f"X{k}"], P[k][f"dW{k}"]
            ring = ring and _aligned(py) and _aligned(px) and ldy * es % 16 == 0 and ldx * es % 16 == 0 and no % 8 == 0 and ni % 8 == 0 \
                and no >= 256 and ni >= 128
            aligned = aligned and ni % 4 == 0 and ldw % 4 == 0 and _aligned(pw)
        pp = _env(case, "POLUS_GEMM_PP", 0) >= 0 and T % 64 == 0 and all(no >= 256 and ni >= 256 for no, ni in probs)
        nkt = (T + 63) // 64
        tiles = [((no + 255) // 256) * ((ni + (255 if pp else 127)) // (256 if pp else 128)) for no, ni in probs]
        if case.split_k > 0:
            asked = [min(case.split_k, nkt)] * len(probs)
        else:                                                            # grouped_splits: one round of the workgroup slots
            slots_xcd, per_xcd, cap = (1 if pp else 2) * NCU // 8, [(t + 7) // 8 for t in tiles], max(nkt // 4, 1)
            asked = [min(max(slots_xcd // sum(per_xcd), 1), cap)] * len(probs)
            used, given = sum(p * a for p, a in zip(per_xcd, asked)), set()
            while True:
                fit = [k for k in range(len(probs)) if k not in given and asked[k] < cap and used + per_xcd[k] <= slots_xcd]
                if not fit:
                    break
                best = max(fit, key=lambda k: (tiles[k], -k))
                given.add(best); asked[best] += 1; used += per_xcd[best]
        if not ring:
            eff = tuple(_dw_single(case, case.dtype, T, no, ni, asked[k], P[k][f"dY{k}"], P[k][f"X{k}"], P[k][f"dW{k}"], case.db)[1]
                        for k, (no, ni) in enumerate(probs))
            return dict(kernel="one_by_one", fused_reduce=False, eff=eff)
        if case.split_k <= 0 and pp and _env(case, "POLUS_DW_STREAMK", 0) and aligned:
            ncu = NCU - _env(case, "POLUS_GEMM_RESERVE_CUS", 0)
            if 0 < _env(case, "POLUS_DW_SK_CUS", 0) < ncu:
                ncu = _env(case, "POLUS_DW_SK_CUS", 0)
            slots = _sk_plan(tiles, T, ncu, _env(case, "POLUS_DW_SK_DELTA", 2))
            if slots:
                return dict(kernel="pp_streamk", fused_reduce=True, eff=(slots,) * len(probs))
        eff = []
        for a in asked:
            kt_per = (nkt + min(a, nkt) - 1) // min(a, nkt)
            eff.append((nkt + kt_per - 1) // kt_per)
        return dict(kernel="pp_grouped" if pp else "ring_grouped", fused_reduce=bool(_env(case, "POLUS_DW_FUSED_REDUCE", 1)) and aligned,
                    eff=tuple(eff))
    return dict(kernel="thin")


# ------------------------------------------------------------------------------------------------ the case list
RING_ENV = (("POLUS_GEMM_PP", -1), ("POLUS_GEMM_RING128", -1))
RING128_ENV = (("POLUS_GEMM_PP", -1), ("POLUS_GEMM_RING128", 1))
PERSIST_ENV = (("POLUS_GEMM_PP", 192), ("POLUS_GEMM_PERSIST", 2), ("POLUS_GEMM_RESERVE_CUS", 224))
MODE_EPIS = ("bias", "act_fwd", "resid", "act_bwd")          # epi_mode 0 .. 3


def _tensors(case):
    """(tensor, kinds that apply) of a case, for the one-at-a-time variants."""
    if case.op == "gemm":
        e = EPI[case.epi]
        epi_kinds = [k for k in EPI_KINDS if k != "pad4" or case.c_dtype == "bf16"]
        t = [("A", OPERAND_KINDS), ("B", OPERAND_KINDS), ("C", epi_kinds)]
        if e.get("resid"):
            t.append(("resid", [k for k in EPI_KINDS if k != "pad4" or case.dtype == "bf16"]))
        if e.get("aux"):
            t.append(("aux", [k for k in EPI_KINDS if k != "pad4" or case.dtype == "bf16"]))
        if e.get("bias"):
            t.append(("bias", ["shift1"]))
        return t
    if case.op == "dw":
        return [("dY", OPERAND_KINDS), ("X", OPERAND_KINDS), ("dW", ("pad16", "cls", "pad1", "shift1"))]
    raise ValueError(case.op)


MIX = {"A": "cls", "B": "pad16", "C": "pad16", "resid": "cls", "aux": "cls", "dY": "cls", "X": "pad16", "dW": "pad16"}


def _with(case, views):
    return Case(**{**case.__dict__, "views": tuple(views)})


def variants(case, level):
    """level "full": all-dense, each tensor alone in each kind that applies to it, everything non-dense at once;
    "ends": all-dense and everything non-dense; "dense": the all-dense case alone."""
    out = [case]
    if level == "dense":
        return out
    tensors = _tensors(case)
    if level == "full":
        out += [_with(case, [(t, k)]) for t, kinds in tensors for k in kinds]
    out.append(_with(case, [(t, MIX[t]) for t, _ in tensors if t in MIX]))
    return out


def _gemm(base, dtype, shape, want, level="ends", **kw):
    return variants(Case(base=base, op="gemm", dtype=dtype, shape=shape, want=want, **kw), level)


def _make_cases():
    c = []
    S, ODD, R, D = (100, 72, 136), (97, 50, 75), (264, 136, 72), (264, 136, 200)
    # V1, f32 engine: 4 layouts, whole chunks and the element path
    for la in ((0, 0), (0, 1), (1, 0), (1, 1)):
        for shape, tag in ((S, "vec"), (ODD, "elem")):
            c += _gemm(f"v1_f32_{la[0]}{la[1]}_{tag}_resid", "f32", shape, "v1", "full" if (la, tag) == ((0, 0), "vec") else "ends", layouts=la, epi="resid")
    for epi in ("alpha", "act_fwd", "act_bwd", "accum"):
        c += _gemm(f"v1_f32_{epi}", "f32", S, "v1", "ends", epi=epi)
    # V1, bf16: by extent (the pad1 / shift1 operands of the ring cases below reach it by a false vector flag)
    for epi in ("resid", "act_fwd", "act_bwd", "accum"):
        c += _gemm(f"v1_bf16_elem_{epi}", "bf16", ODD, "v1", epi=epi)
    c += _gemm("v1_bf16_f32c_11", "bf16", ODD, "v1", layouts=(1, 1), c_dtype="f32", epi="alpha_accum")
    # V1 + dropout
    for dt in ("f32", "bf16"):
        c += _gemm(f"v1_{dt}_drop", dt, S, "v1", "full" if dt == "bf16" else "ends", epi="drop")
        c += _gemm(f"v1_{dt}_drop_elem", dt, ODD, "v1", epi="drop_only")
    # V1 + REDUCE_PLAIN; an epilogue with split_k that falls back to one slice
    c += _gemm("v1_f32_split3", "f32", S, "v1", split_k=3, epi="alpha_accum")
    c += _gemm("v1_bf16_f32c_split3", "bf16", S, "v1", split_k=3, c_dtype="f32", epi="bias")
    c += _gemm("v1_bf16_split3_one_slice", "bf16", S, "v1", split_k=3, epi="resid")
    # RING, run-time epilogue
    c += _gemm("ring_rt_f32c", "bf16", R, "ring", c_dtype="f32", epi="alpha")
    c += _gemm("ring_rt_accum", "bf16", R, "ring", "full", epi="accum")
    for la in ((0, 1), (1, 0), (1, 1)):
        c += _gemm(f"ring_rt_{la[0]}{la[1]}", "bf16", R, "ring", layouts=la, epi="resid")
    # RING 256 x 128 and RING128 with compile-time epilogues, and with dropout
    for want, env in (("ring", RING_ENV), ("ring128", RING128_ENV)):
        for epi in MODE_EPIS:
            c += _gemm(f"{want}_{epi}", "bf16", R, want, "full" if epi == "resid" or (epi, want) == ("act_fwd", "ring") else "ends", env=env, epi=epi)
        c += _gemm(f"{want}_alpha", "bf16", R, want, "dense", env=env, epi="alpha")
        dwant = "ring_drop" if want == "ring" else want
        c += _gemm(f"{dwant}_drop", "bf16", R, dwant, "full" if want == "ring" else "ends", env=env, epi="drop")
        # dropout without a residual has no compile-time epilogue class (mode -1), which the 128 x 128 tile needs
        c += _gemm(f"ring_drop_only_{'ring128_on' if want == 'ring128' else 'ring128_off'}", "bf16", R, "ring_drop", env=env, epi="drop_only")
    # PP 256 / 192: one and three K tiles
    for tn in (256, 192):
        env = (("POLUS_GEMM_PP", tn),)
        for epi in MODE_EPIS + ("drop",):
            c += _gemm(f"pp{tn}_{epi}_k192", "bf16", (264, 264, 192), "pp", "full" if epi == "resid" else "ends", env=env, epi=epi)
            c += _gemm(f"pp{tn}_{epi}_k64", "bf16", (264, 264, 64), "pp", "dense" if epi != "drop" else "ends", env=env, epi=epi)
    # PP_PERSIST: 5 x 8 = 40 tiles of 256 x 192 on 32 workgroups
    for epi in MODE_EPIS + ("drop",):
        c += _gemm(f"pp_persist_{epi}", "bf16", (1032, 1352, 64), "pp_persist", "ends" if epi in ("resid", "drop") else "dense", env=PERSIST_ENV, epi=epi)
    # RING slabs + REDUCE_PLAIN (the dW form) and + REDUCE_EPI
    c += _gemm("ring_slabs_plain", "bf16", D, "ring", "full", layouts=(1, 1), c_dtype="f32", split_k=3)
    c += _gemm("ring_slabs_plain_alpha_accum", "bf16", D, "ring", layouts=(1, 1), c_dtype="f32", split_k=3, epi="alpha_accum")
    for epi in MODE_EPIS + ("alpha", "drop", "drop_only"):
        c += _gemm(f"ring_slabs_epi_{epi}", "bf16", D, "ring", "full" if epi == "resid" else "ends", split_k=3, epi=epi)
    # gelu / swish / tanh, forward and backward: one case per route
    for route, shape, env, kw in (("v1_f32", S, (), {}), ("v1_bf16", ODD, (), {}), ("ring", R, RING_ENV, {}), ("ring128", R, RING128_ENV, {}),
                                  ("pp", (264, 264, 192), (("POLUS_GEMM_PP", 256),), {}), ("pp", (264, 264, 192), (("POLUS_GEMM_PP", 192),), {}),
                                  ("pp_persist", (1032, 1352, 64), PERSIST_ENV, {}), ("ring", D, (), dict(split_k=3))):
        for act in ("gelu", "swish", "tanh"):
            for epi in ("act_fwd", "act_bwd"):
                tag = f"{route}{dict(env).get('POLUS_GEMM_PP', '') if route == 'pp' else ''}{'_slabs_epi' if kw else ''}"
                want = "v1" if route.startswith("v1") else route
                c += _gemm(f"{tag}_{act}_{epi}", "f32" if route == "v1_f32" else "bf16", shape, want, "ends" if shape[0] < 1000 and (epi, act) == ("act_fwd", "gelu") else "dense",
                           env=env, epi=epi, act=act, **kw)
    # polus_dense_bwd_params: ring with db, and the fallbacks
    DW = (200, 264, 136)
    for sk in (1, 3):
        for acc in (False, True):
            c += variants(Case(base=f"dw_ring_split{sk}{'_accum' if acc else ''}", op="dw", dtype="bf16", shape=DW, want="ring", split_k=sk, accumulate=acc),
                          "full" if (sk, acc) == (3, True) else "ends")
    c += variants(Case(base="dw_fallback_no_db", op="dw", dtype="bf16", shape=DW, want="fallback", split_k=3, db=False), "ends")
    for dt in ("bf16", "f32"):
        c += variants(Case(base=f"dw_fallback_small_{dt}", op="dw", dtype=dt, shape=(75, 50, 97), want="fallback", split_k=2 if dt == "bf16" else 1, accumulate=dt == "f32"), "ends")
    # grouped dW: two problems each (three and five where the hand-out of slices is to show)
    G = lambda base, T, probs, want, views=(), **kw: Case(base=base, op="dwg", dtype="bf16", shape=(T, probs), want=want, views=views, **kw)
    for kind in ("dense", "pad16", "pad1"):
        v = () if kind == "dense" else (("dW0", kind), ("dW1", kind))
        c.append(G("dwg_ring", 192, ((264, 264), (264, 136)), "ring_grouped", v, split_k=3))
        c.append(G("dwg_ring_t200", 200, ((264, 264), (264, 264)), "ring_grouped", v, split_k=2, accumulate=True))
        c.append(G("dwg_pp", 192, ((264, 264), (264, 264)), "pp_grouped", v, split_k=3))
        c.append(G("dwg_pp_one_slice", 192, ((264, 264), (264, 264)), "pp_grouped", v, split_k=1, accumulate=True))
        c.append(G("dwg_streamk", 768, ((264, 264), (264, 264)), "pp_streamk", v, split_k=0,
                   env=(("POLUS_DW_STREAMK", 1), ("POLUS_DW_SK_CUS", 12))))
    c.append(G("dwg_pp", 192, ((264, 264), (264, 264)), "pp_grouped", (("dY0", "cls"), ("X0", "pad16"), ("dY1", "pad16"), ("X1", "cls")), split_k=3))
    c.append(G("dwg_pp_unfused", 192, ((264, 264), (264, 264)), "pp_grouped", split_k=3, env=(("POLUS_DW_FUSED_REDUCE", 0),)))
    c.append(G("dwg_pp_no_db", 192, ((264, 264), (264, 264)), "pp_grouped", split_k=3, db=False))
    # split_k = 0, the library chooses the slices (grouped_splits); the handout cases are the smallest at which its extra slice
    # for the problems with most tiles shows in the report: eff (11, 11, 10) and (13, 13, 13, 13, 11)
    c.append(G("dwg_pp_auto", 768, ((264, 264), (264, 264)), "pp_grouped", split_k=0))
    c.append(G("dwg_ring_auto", 768, ((264, 264), (264, 136)), "ring_grouped", split_k=0))
    c.append(G("dwg_pp_auto_handout", 3520, ((264, 264),) * 3, "pp_grouped", split_k=0))
    c.append(G("dwg_ring_auto_handout", 3328, ((264, 136), (264, 264)) * 2 + ((264, 136),), "ring_grouped", split_k=0))
    c.append(G("dwg_one_by_one", 192, ((264, 264), (264, 264)), "one_by_one", (("dY1", "pad1"),), split_k=3))
    c.append(G("dwg_one_by_one", 192, ((264, 264), (264, 264)), "one_by_one", (("X0", "shift1"),), split_k=3))
    c.append(G("dwg_one_by_one_small", 192, ((264, 264), (120, 264)), "one_by_one", split_k=2, accumulate=True))
    c.append(G("dwg_one_by_one_no_db", 200, ((264, 136), (50, 97)), "one_by_one", split_k=2, db=False))
    # dense_thin
    for dt in ("bf16", "f32"):
        for H, C, ydt in ((128, 3, "f32"), (264, 8, dt), (264, 1, "f32"), (128, 8, dt)):
            T = lambda op, views=(), **kw: Case(base=f"{op}_{dt}_h{H}_c{C}_y{ydt}", op=op, dtype=dt, shape=(37, H, C), want="thin", c_dtype=ydt,
                                                views=views, **kw)
            c.append(T("thin_fwd"))
            c.append(T("thin_fwd", (("x", "cls"), ("y", "pad1"))))
            c.append(T("thin_fwd", (("x", "pad16"), ("w", "pad16"), ("y", "pad16"))))
            c.append(T("thin_bwd"))
            c.append(T("thin_bwd", (("x", "cls"), ("dy", "pad1"), ("dx", "pad16"), ("dw", "pad1"))))
            c.append(T("thin_bwd", (("x", "pad16"), ("dy", "pad16"), ("w", "cls"), ("dx", "cls"), ("dw", "pad16")), accumulate=True))
        T = lambda op, views: Case(base=f"{op}_{dt}_refused", op=op, dtype=dt, shape=(37, 128, 3), want="thin", views=views, refused=True)
        c += [T("thin_fwd", (("x", "pad1"),)), T("thin_fwd", (("x", "shift1"),)), T("thin_fwd", (("w", "shift1"),)),
              T("thin_bwd", (("x", "pad1"),)), T("thin_bwd", (("dx", "shift1"),)), T("thin_bwd", (("w", "pad1"),))]
    names = [x.name for x in c]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return c


CASES = _make_cases()
BY_NAME = {c.name: c for c in CASES}


def dense_twin(case):
    return BY_NAME.get(case.base + "/dense")


# ------------------------------------------------------------------------------------------------ what both test files call
class switches:
    """with switches(case): the case's POLUS_* switches are set, and unset again on the way out."""

    def __init__(self, case):
        self.case = case

    def __enter__(self):
        from polus_amd import ops
        for k, v in self.case.env:
            ops.set_env(k, v)

    def __exit__(self, *exc):
        from polus_amd import ops
        for k, _ in self.case.env:
            ops.set_env(k)
        return False


def gemm_keywords(case):
    """The scalar keywords of ops.gemm / ops.gemm_route for a gemm case (the tensors are the caller's)."""
    e = EPI[case.epi]
    flags = (1 if e.get("accum") else 0) | (2 if e.get("aux") == "w" else 0) | (4 if e.get("aux") == "r" else 0)
    return dict(a_layout=case.layouts[0], b_layout=case.layouts[1], alpha=e.get("alpha", 1.0), act=case.act, flags=flags,
                split_k=case.split_k, drop_p=DROP_P if e.get("drop") else 0.0, seed=case.drop_seed)
