"""Cases for the layers (polus_amd/layers.py Dense and Dropout, the shadow handling of polus_amd/tensor.py), shared by the GPU
file that drives every dispatch path (test_layers_gpu.py) and by the CPU check of the reference and of the case table
(test_layer_cases_cpu.py).  No GPU needed to import.

Dense.forward chooses between two implementations:
  thin   dense_thin.hip, a wave per row: no activation, x with unit column stride, a 16-byte aligned base and row stride,
         POLUS_DENSE_THIN != 0 and polus_dense_thin_supported(dtype, H, C)
  gemm   polus_gemm (+ aux / act_bwd for an activation), polus_dense_bwd_params and the dX GEMM otherwise
Dense.backward chooses again: the thin backward after a thin forward when no dx_resid is given and dy is f32 or in the compute
dtype, the GEMM backward otherwise (a dy of another dtype is cast to the compute dtype first).

The reference is NumPy in float64 on the operands the device holds (already rounded to the engine's dtype), with the
roundings of the path under test applied where the path applies them:
  dy_dtype   the dtype in which dy reaches the contraction: the thin backward reads an f32 dy as it is, the GEMM backward of
             the bf16 engine casts it to bf16 first
  u_dtype    an activated layer keeps its pre-activation u in the compute dtype (the aux output of the forward GEMM) and
             act_bwd reads it from there
  du_dtype   act_bwd writes du = dy * act'(u) in the compute dtype

Bounds, none of them taken from the layers' output (max error / max|ref|):
  y, dx      tests.util.TOL of the dtype the tensor is stored in
  dW, db     thin path: 2e-5 (test_kernels_gpu.py test_dense_thin); GEMM path: test_dense_bwd_params' 3e-5 / 1e-4 in f32,
             2e-3 / 2e-3 in bf16
Two paths are held to each other within the sum of their two bounds.

Shapes.  The heads the product builds and the edges of the gate, plus (520, 5): without it no case reaches the CP = 8
instantiations with the larger chunk count (bf16 <8, 2>, f32 <8, 4>), which need 5..8 units and more than 512 features.
(1032, 4) is outside the thin kernels in BOTH engines (bf16: three 512-wide chunks, f32: five 256-wide chunks), as the library's
own gate says (test_layer_cases_cpu.py holds the restatement to it)."""
from dataclasses import dataclass, field

import numpy as np
import torch

from oracle import bert as ob
from tests.rowwise_cases import ACTS, act_grad
from tests.util import TOL, rounded

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
ES = {"f32": 4, "bf16": 2}
ENGINES = ("f32", "bf16")

# dense_thin.hip, restated
THIN_TW = 4                    # waves (= rows in flight) per workgroup
THIN_MAX_BLOCKS = 512
THIN_VEC = {"f32": 4, "bf16": 8}
THIN_MAX_NCH = {"f32": 4, "bf16": 2}
THIN_INSTANCES = {"bf16": {(cp, nch) for cp in (4, 8) for nch in (1, 2)},
                  "f32": {(cp, nch) for cp in (4, 8) for nch in (2, 4)}}

THIN_PARAM_TOL = 2e-5
GEMM_DW_TOL = {"f32": 3e-5, "bf16": 2e-3}
GEMM_DB_TOL = {"f32": 1e-4, "bf16": 2e-3}


# ------------------------------------------------------------------------------------------------- the gate, restated
def thin_nch(dtype, H):
    span = 64 * THIN_VEC[dtype]
    return (H + span - 1) // span


def thin_supported(dtype, H, C):
    """polus_dense_thin_supported(dtype, H, C)."""
    if dtype not in THIN_VEC:
        return False
    vec = THIN_VEC[dtype]
    return 1 <= C <= 8 and H >= vec and H % vec == 0 and thin_nch(dtype, H) <= THIN_MAX_NCH[dtype]


def thin_instance(dtype, H, C):
    """(CP, NCH) of the kernel THIN_DISPATCH picks for a supported shape."""
    assert thin_supported(dtype, H, C)
    n = thin_nch(dtype, H)
    nch = (1 if n <= 1 else 2) if dtype == "bf16" else (2 if n <= 2 else 4)
    return (4 if C <= 4 else 8), nch


def thin_blocks(rows):
    """Workgroups of a thin launch: at least two rows per wave, at most THIN_MAX_BLOCKS."""
    return max(1, min((rows + 2 * THIN_TW - 1) // (2 * THIN_TW), THIN_MAX_BLOCKS))


def thin_sweeps(rows):
    """(trips of the longest wave round the grid-stride loop, rows of the last trip)."""
    per = thin_blocks(rows) * THIN_TW
    return (rows + per - 1) // per, (rows - 1) % per + 1


def layer_thin(dtype, H, C, activation=None, col_stride=1, base_elems=0, row_stride=None, env=None):
    """The `_thin` Dense.forward must arrive at for an x [rows, H] on the device that starts `base_elems` elements into a
    256-byte aligned allocation with the given strides (in elements), under POLUS_DENSE_THIN = env (None: unset)."""
    rs = H if row_stride is None else row_stride
    es = ES[dtype]
    return bool(not activation and col_stride == 1 and (base_elems * es) % 16 == 0 and (rs * es) % 16 == 0 and
                env != "0" and thin_supported(dtype, H, C))


# ------------------------------------------------------------------------------------------------- the reference
def act_fwd(act, u):
    if not act:
        return u
    if act == "gelu":
        return ob.gelu(u)
    if act == "swish":
        return ob.swish(u)
    if act == "relu":
        return np.maximum(u, 0.0)
    assert act == "tanh", act
    return np.tanh(u)


def _round(a, dtype):
    return a if dtype is None else rounded(a, DT[dtype] if isinstance(dtype, str) else dtype)


def dense_reference(x, w, b, dy=None, act=None, resid=None, dy_dtype=None, u_dtype=None, du_dtype=None):
    """float64 Dense on the values the device holds: y = act(x W^T + b); with dy also du = dy * act'(u), dx = du W (+ resid),
    dw = du^T x, db = sum over rows of du.  *_dtype ("f32" / "bf16" / None): the tensor passes through that dtype first."""
    u = x @ w.T
    if b is not None:
        u = u + b
    out = {"u": u, "y": act_fwd(act, u)}
    if dy is None:
        return out
    du = _round(dy, dy_dtype)
    if act:
        du = _round(du * act_grad(act, _round(u, u_dtype)), du_dtype)
    dx = du @ w
    if resid is not None:
        dx = dx + resid
    out.update(du=du, dx=dx, dw=du.T @ x, db=du.sum(0))
    return out


def path_roundings(engine, thin, dy_dtype, act=None):
    """The keyword roundings of dense_reference for a backward on the thin / GEMM path of `engine` fed a dy of dy_dtype."""
    if thin:
        assert not act and dy_dtype in ("f32", engine)
        return {"dy_dtype": dy_dtype}
    kw = {"dy_dtype": dy_dtype if ES[dy_dtype] <= ES[engine] else engine}     # cast to the compute dtype (widening is exact)
    if act:
        kw.update(u_dtype=engine, du_dtype=engine)
    return kw


def bounds(engine, thin, y_dtype=None):
    """Relative bounds (of max|ref|) of the four outputs on one path."""
    p = THIN_PARAM_TOL
    return {"y": TOL[DT[y_dtype or engine]], "dx": TOL[DT[engine]],
            "dw": p if thin else GEMM_DW_TOL[engine], "db": p if thin else GEMM_DB_TOL[engine]}


# ------------------------------------------------------------------------------------------------- the case table
SHAPES = ((128, 3),        # one chunk per lane, CP = 4
          (264, 8),        # ragged last chunk, CP = 8
          (768, 4),        # the BERT head
          (1024, 1),       # the widest thin case, and the cross-encoder head
          (768, 10),       # just past the unit limit: the GEMM path (the tutorial's Dense(10))
          (1032, 4),       # just past the feature limit of the bf16 kernels (and far past the f32 ones'): the GEMM path
          (520, 5))        # CP = 8 with two bf16 chunks (the second ragged) / three of four f32 chunks
ROWS = (5,                 # one workgroup, its first wave takes a second row
        37,
        513,
        4099)              # past the 512-workgroup cap: three trips round the grid-stride loop, the last with 3 rows


@dataclass
class DenseCase:
    engine: str
    H: int
    C: int
    rows: int
    use_bias: bool = True
    out: str = "f32"           # "f32": out_dtype=torch.float32 (logits feeding a loss); "compute": the layer's default
    thin: bool = field(init=False)

    def __post_init__(self):
        self.thin = layer_thin(self.engine, self.H, self.C)

    @property
    def y_dtype(self):
        return "f32" if self.out == "f32" else self.engine

    @property
    def instance(self):
        return thin_instance(self.engine, self.H, self.C) if self.thin else None

    @property
    def seed(self):
        return (self.rows * 7919 + self.H * 31 + self.C * 3 + (5 if self.engine == "bf16" else 0)) & 0xFFFFFFFF

    @property
    def name(self):
        return (f"{'thin' if self.thin else 'gemm'}-{self.engine}-H{self.H}-C{self.C}-r{self.rows}" +
                ("" if self.use_bias else "-nobias") + ("" if self.out == "f32" else "-out_compute"))


def _cases():
    out = [DenseCase(e, H, C, rows) for e in ENGINES for H, C in SHAPES for rows in ROWS]
    # no bias: no db, a null bias pointer in the thin forward
    out += [DenseCase(e, H, C, 37, use_bias=False) for e in ENGINES for H, C in ((128, 3), (264, 8), (768, 10))]
    # the layer's default output dtype (the compute dtype); in the f32 engine that is the same layer as out="f32"
    out += [DenseCase("bf16", H, C, 37, out="compute") for H, C in SHAPES]
    out += [DenseCase("bf16", 768, 4, 4099, out="compute"), DenseCase("bf16", 264, 8, 513, use_bias=False, out="compute")]
    return out


CASES = _cases()


def dense_inputs(engine, rows, H, C, seed, use_bias=True):
    """x, w, b (None without bias), dy as float64; x and w already rounded to the engine's dtype, b and dy to f32.  Scales as
    in test_kernels_gpu.py test_dense_thin, whose bounds are used here: x ~ N(0, 1), w, dy ~ 0.1 N(0, 1)."""
    r = np.random.Generator(np.random.PCG64(seed))
    x = rounded(r.standard_normal((rows, H)), DT[engine])
    w = rounded(r.standard_normal((C, H)) * 0.1, DT[engine])
    b = rounded(r.standard_normal(C), torch.float32)
    dy = rounded(r.standard_normal((rows, C)) * 0.1, torch.float32)
    return x, w, (b if use_bias else None), dy


__all__ = ["ACTS", "CASES", "DenseCase", "dense_inputs", "dense_reference"]
